"""Timings of the PuLID path on one MI355X (bench.py stays the flagship benchmark and is not involved).

1. One identity cross-attention call at T in {1024, 4096}, C = 3072, H = 16, N = 32, bf16 and fp16, three arms on the same tensors:
   the fused op (``svdq_pulid_ca``: the stats-only pass and the two launches of the folded kernel), the composed arm built from what the
   library had (torch LayerNorm, ``F.linear`` for Q, ``svdq_ip_attention`` on 16 heads and 32 keys, ``F.linear`` for the output, the
   strength multiply) and the reference's torch-op sequence (``PerceiverAttentionCA.forward`` and the multiply).  K / V and the fold are
   made once per embeddings tensor and are in none of the three.  The accuracy ratios of the fused module against the torch-op sequence
   (float64 reference composition) are recorded at T = 513.
2. A FLUX.1-dev-shaped 1024 x 1024 step with synthetic weights in the default mode: plain (modules detached), with the 20 modules on the
   fused arm and on the torch-op arm (``pulid_fused`` off) inside the fused blocks.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_pulid.py [--repeats 7] [--inner 3] [--layers 19 38] [--out profiles/pulid.txt]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_ip_attention import alternate, line  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--layers", type=int, nargs=2, default=(19, 38))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd.models import pulid
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.ops.attention import ip_attention, pulid_ca
    from nunchaku_amd.ops.elementwise import residual_gate_stats
    from tests import pulid_ref as ref

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner} (call: x 10), versions alternated, "
             "times between device events, no counter run was made"]

    # ---- 1. one call ----------------------------------------------------------------------------------------------------------------
    C, H, N, KV, weight = 3072, 16, 32, 2048, 0.8
    lines.append(f"identity cross-attention call, C = {C}, H = {H}, N = {N}, kv_dim {KV}, id_weight {weight}; fold and K / V made beforehand")
    with torch.no_grad():
        for dtype in ("bf16", "fp16"):
            td = ref.TD[dtype]
            mod = ref.make_module(C, H, KV, 128, seed=1, dtype=td, device=dev)
            emb = torch.randn(1, N, KV, generator=torch.Generator().manual_seed(2)).to(td).to(dev)
            fold = mod.fold(emb)
            k, v = mod.to_kv(mod.norm1(emb[0])).chunk(2, dim=-1)
            k, v = k.contiguous(), v.contiguous()
            for T in (1024, 4096):
                x = ref.stream_inputs(T, C, 5, td, dev)
                out = torch.empty_like(x)
                stats = residual_gate_stats(x, eps=1e-5)[1]

                def composed():
                    q = F.linear(F.layer_norm(x, (C,), mod.norm2.weight, mod.norm2.bias, 1e-5), mod.to_q.weight)
                    return F.linear(ip_attention(q, k, v, H, out_scale=weight), mod.to_out.weight)

                versions = {
                    "fused op (stats pass + svdq_pulid_ca)": lambda: pulid_ca(x, fold, out_scale=weight, out=out),
                    "fused op, statistics given": lambda: pulid_ca(x, fold, out_scale=weight, stats=stats, out=out),
                    "composed arm (LN, linear, svdq_ip_attention, linear)": composed,
                    "torch-op sequence (module forward, x weight)": lambda: weight * mod(emb, x[None]),
                }
                t = alternate(versions, args.repeats, args.inner * 10)
                med = {n_: statistics.median(xs) for n_, xs in t.items()}
                names = list(versions)
                flop_fold, flop_comp = 4.0 * T * C * H * 32, 4.0 * T * C * H * 128
                lines.append(f"  {dtype}, T = {T}: MFMA work folded {flop_fold / 1e9:.1f} GFLOP, the composed arm's two GEMMs {flop_comp / 1e9:.1f} GFLOP")
                for n_ in names:
                    extra = ""
                    if n_ == names[1]:
                        extra = f"  {flop_fold / (med[n_] * 1e-3) / 1e12:.0f} TFLOP/s"
                    if n_ == names[2]:
                        extra = f"  fused / composed = {med[names[0]] / med[n_]:.2f}"
                    if n_ == names[3]:
                        extra = f"  fused / torch = {med[names[0]] / med[n_]:.2f}"
                    lines.append(line("    " + n_, t[n_], extra))
            lat = ref.stream_inputs(513, C, 11, td, dev)
            want = ref.compose64(mod, emb, lat)
            e_f = (mod.forward_fused(emb, lat).double().cpu() - want).abs()
            e_t = (mod(emb, lat[None])[0].double().cpu() - want).abs()
            lines.append(f"  {dtype}, T = 513: error against the float64 composition: fused max {e_f.max():.4g} mean {e_f.mean():.4g}; torch ops max "
                         f"{e_t.max():.4g} mean {e_t.mean():.4g}; ratios max {e_f.max() / e_t.max():.3f} mean {e_f.mean() / e_t.mean():.3f}")

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
    count = pulid.pulid_module_count(model)
    pulid.attach_pulid(model, ref.module_state_dict(count, model.dim, H, KV, seed=3, encoder=False))
    emb = torch.randn(1, N, KV, generator=g, device=dev, dtype=torch.bfloat16)
    lines.append(f"FLUX.1-dev-shaped step, {nj} + {ns} blocks, 1024 x 1024, {t_txt} text tokens, bf16, synthetic weights, default mode, {count} PuLID modules")

    def fused():
        return model.engine_forward(*inputs, id_embeddings=emb, id_weight=weight)

    def torch_arm():
        model.pulid_fused = False
        try:
            return model.engine_forward(*inputs, id_embeddings=emb, id_weight=weight)
        finally:
            del model.pulid_fused

    with torch.no_grad():
        t = alternate({"plain (no id_embeddings)": lambda: model.engine_forward(*inputs), "PuLID, fused arm": fused,
                       "PuLID, torch-op arm in fused blocks": torch_arm}, args.repeats, args.inner)
    for n_, xs in t.items():
        lines.append(line("  " + n_, xs))
    med = {n_: statistics.median(xs) for n_, xs in t.items()}
    base = med["plain (no id_embeddings)"]
    lines.append(f"  cost over the plain step (medians): fused arm {med['PuLID, fused arm'] - base:+.3f} ms ({(med['PuLID, fused arm'] - base) / count * 1e3:.0f} us "
                 f"per module), torch-op arm {med['PuLID, torch-op arm in fused blocks'] - base:+.3f} ms; spread of plain (max - min) "
                 f"{max(t['plain (no id_embeddings)']) - min(t['plain (no id_embeddings)']):.3f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
