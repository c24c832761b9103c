"""Timings of the T5 encoder's attention on one MI355X (bench.py stays the flagship benchmark and is not involved).

``svdq_attention_d64_bias`` (one launch: Q, K, V read in place from the projections' token-major outputs, the relative position bias as one
Toeplitz vector per head, the padding mask as a per-key bias) at (B, T = N, H) = (1, 512, 64), (1, 256, 64), (2, 512, 64), in bf16 and fp16, against

  (a) transformers' eager sequence in the same run: the transposed views, the ``[B, H, T, N]`` score matmul, the add of the materialised
      ``[1, H, T, N]`` position bias, the add of the ``[B, 1, 1, N]`` mask, softmax, the second matmul, the transpose + copy back;
  (b) ``F.scaled_dot_product_attention`` with position bias + mask materialised as ``attn_mask`` (the add is inside the timing: it happens per layer).

Then (without ``--graph``) the 24-layer T5-XXL-shaped 4-bit encoder (d_model 4096, d_ff 10240, 64 heads, random weights) at 512 tokens, on the
fused attention and on transformers' eager attention.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_t5_attention.py [--repeats 7] [--inner 20] [--graph] [--out profiles/t5_attention.txt] [--no-encoder]

``--graph`` times each version as the replay of a captured graph of ``inner`` calls: the device's time without the host's issue time.
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_sdxl_attention import alternate, line  # noqa: E402

SHAPES = [(1, 512, 64), (1, 256, 64), (2, 512, 64)]  # (B, T = N, H)


def xxl_encoder(dev, layers=24):
    """a T5-XXL-shaped encoder with random weights, every nn.Linear a W4Linear (group 128)"""
    import transformers

    from nunchaku_amd.models.text_encoders import W4Linear

    cfg = transformers.T5Config(vocab_size=256, d_model=4096, d_kv=64, d_ff=10240, num_layers=layers, num_heads=64, feed_forward_proj="gated-gelu",
                                dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    with torch.device(dev):
        model = transformers.T5EncoderModel(cfg).bfloat16().eval()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn_like(p.float()).mul(1.0 / 64).bfloat16())
        for mod in list(model.modules()):
            for cname, child in list(mod.named_children()):
                if isinstance(child, torch.nn.Linear):
                    setattr(mod, cname, W4Linear.from_linear(child, group_size=128))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph", action="store_true", help="time replays of a captured graph of --inner calls (device time without the host's issue time)")
    ap.add_argument("--no-encoder", action="store_true", help="skip the 24-layer encoder")
    args = ap.parse_args()

    from nunchaku_amd.models.text_encoders.t5_encoder import ATTENTION_NAME, register_fused_attention
    from nunchaku_amd.ops import attention_d64_bias

    if not torch.cuda.is_available():
        raise SystemExit("bench_t5_attention: no GPU: a timing needs the MI355X (nothing is measured on the CPU)")
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
    emit("T5 attention at head dimension 64, relative position bias + padding mask (the last quarter of the keys padded); "
         + ("times are replays of a captured graph of the calls, per call: the device's time without the host's issue time; " if args.graph else
            "times are call times between device events, not kernel times from a trace; ") + "no counter run was made")
    g = torch.Generator(device=dev).manual_seed(0)
    for dtype in (torch.bfloat16, torch.float16):
        for B, T, H in SHAPES:
            hd, N = H * 64, T
            q, k, v = (torch.randn(B, T, hd, device=dev, generator=g).to(dtype) for _ in range(3))
            rel = 2.0 * torch.randn(H, 2 * T - 1, device=dev, generator=g)
            idx = torch.arange(N, device=dev)[None, :] - torch.arange(T, device=dev)[:, None] + T - 1
            pb = rel[:, idx][None].to(dtype)                                # [1, H, T, N]: what compute_bias hands the layers
            kb = torch.zeros(B, N, device=dev)
            kb[:, N - N // 4:] = torch.finfo(dtype).min
            mask = kb.to(dtype)[:, None, None, :]                           # [B, 1, 1, N]
            out = torch.empty(B, T, hd, device=dev, dtype=dtype)

            def kernel():
                return attention_d64_bias(q, k, v, H, rel, kb, out=out)

            def heads(t):
                return t.view(B, -1, H, 64).transpose(1, 2)

            def eager():
                w = torch.matmul(heads(q), heads(k).transpose(2, 3)) * 1.0
                w = F.softmax(w + pb + mask, dim=-1)
                return torch.matmul(w, heads(v)).transpose(1, 2).contiguous().reshape(B, T, hd)

            def sdpa():
                return F.scaled_dot_product_attention(heads(q), heads(k), heads(v), attn_mask=pb + mask, scale=1.0).transpose(1, 2).reshape(B, T, hd)

            ref = eager().float()
            diff = (kernel().float() - ref).abs().max().item()
            t = alternate({"kernel": kernel, "eager": eager, "sdpa": sdpa}, args.repeats, args.inner, args.graph)
            med = {k_: statistics.median(xs) for k_, xs in t.items()}
            name = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]
            emit(f"{name} (B, T = N, H) = ({B}, {T}, {H}): max |kernel - eager| = {diff:.3g} (max |eager| {ref.abs().max().item():.3g})")
            emit(line("  svdq_attention_d64_bias (1 launch)", t["kernel"],
                      f"  kernel / eager = {med['kernel'] / med['eager']:.3f}; kernel / SDPA = {med['kernel'] / med['sdpa']:.3f}"))
            emit(line("  (a) transformers' eager sequence", t["eager"]))
            emit(line("  (b) SDPA, bias + mask as attn_mask", t["sdpa"]))
            del q, k, v, out, ref, pb
    if not args.no_encoder and not args.graph:  # (transformers' eager mask function copies a scalar from the host: its encoder cannot be captured)
        assert register_fused_attention()
        model = xxl_encoder(dev)
        ids = torch.randint(0, 256, (1, 512), device=dev, generator=g)
        pad = torch.ones(1, 512, dtype=torch.long, device=dev)
        pad[:, 384:] = 0
        for label, am in (("no mask", None), ("padding mask (384 of 512 real)", pad)):
            def run(name):
                def fn():
                    model.config._attn_implementation = name
                    with torch.no_grad():
                        return model(input_ids=ids, attention_mask=am).last_hidden_state
                return fn

            t = alternate({"fused": run(ATTENTION_NAME), "eager": run("eager")}, args.repeats, max(1, args.inner // 10))
            med = {k_: statistics.median(xs) for k_, xs in t.items()}
            emit(f"T5-XXL-shaped 4-bit encoder, 24 layers, 512 tokens, bf16, {label}: fused / eager = {med['fused'] / med['eager']:.3f}")
            emit(line("  encoder on svdq_attention_d64_bias", t["fused"]))
            emit(line("  encoder on transformers' eager attention", t["eager"]))


if __name__ == "__main__":
    main()
