"""Timings of Z-Image's two glue kernels and of a whole Z-Image block on one MI355X (bench.py stays the flagship benchmark and is not involved).

Part 1, ``svdq_sandwich_norm`` (one launch) at Z-Image's C = 3840, B = 1, T in {1024, 4096, 4352} tokens, both dtypes, in the three modes a
stack runs it in --

  open   out_mod = rms(res, w_pre) * scale                                                  (reads res; writes out_mod)
  mid    out = res + gate * rms(a, w_post);  out_mod = rms(out, w_pre) * scale              (reads a, res; writes out, out_mod)
  close  out = res + gate * rms(a, w_post)                                                  (reads a, res; writes out)

-- against (a) the 16-bit torch-op sequence it replaces (diffusers' RMSNorm: pow, mean, rsqrt, two multiplies and a cast per norm; the
modulation, the gate and the residual one op each) and (b) its byte bound: the 16-bit elements it must read and write at the chip's measured
copy figure (weights and per-sample vectors left out).

Part 2, ``svdq_qk_norm_rope`` (one launch) at H = 30 heads of 128 on the packed [T, 11520] projection, against (a) the reference processor's
torch ops -- two RMSNorms over the heads, the rotation through fp32 complex tensors, and the one copy our attention needs besides (V
transposed) -- and (b) its byte bound: Q, K, V read, Q, K and V^T written, the fp32 freqs read.

Part 3, a block (dim 3840, 30 heads, hidden 10240, rank 32, random weights, batch 1): ``NunchakuZImageTransformerBlock.forward`` (fused: three
sandwich passes, one QK pass, ``svdq_attention``) against the same block composed from 16-bit torch ops around the same ``SVDQW4A4Linear`` s
(diffusers' order of operations, ``F.scaled_dot_product_attention``).

Outputs are compared before anything is timed.  Event-bracketed, warm; the versions alternate inside one process and the whole round is
repeated: min / median / max per version.

    python tools/bench_zimage.py [--repeats 7] [--inner 20] [--out profiles/zimage.txt] [--skip-block]
"""

import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X
C, H, HIDDEN = 3840, 30, 10240
TOKENS = [1024, 4096, 4352]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS = 1e-5
MODES = {"open": (False, True), "mid": (True, True), "close": (True, False)}  # name -> (a given, out_mod asked for)


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


def rmsnorm(x, w, eps=EPS):
    """diffusers' RMSNorm.forward with a 16-bit weight"""
    variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    return (x * torch.rsqrt(variance + eps)).to(w.dtype) * w


def rope(x_in, freqs_cis):
    """the reference processor's apply_rotary_emb: x_in [B, T, H, 128], freqs_cis [B, T, 64] complex64"""
    x = torch.view_as_complex(x_in.float().reshape(*x_in.shape[:-1], -1, 2))
    return torch.view_as_real(x * freqs_cis.unsqueeze(2)).flatten(3).type_as(x_in)


def bench_sandwich(args, emit, dev):
    from nunchaku_amd.ops import sandwich_norm

    emit(f"svdq_sandwich_norm, C = {C}, B = 1, one launch per call; byte bound = 2 * T * C * (tensors read + written) bytes at {COPY_TBS} TB/s; "
         "no counter run was made")
    g = torch.Generator(device=dev).manual_seed(0)
    for dname, dt in DTYPES.items():
        rnd = lambda *s, scale=1.0, shift=0.0: (scale * torch.randn(*s, device=dev, generator=g) + shift).to(dt)
        for T in TOKENS:
            res, a = rnd(1, T, C), rnd(1, T, C, scale=3.0)
            w_post, w_pre = rnd(C, scale=0.1, shift=1.0), rnd(C, scale=0.1, shift=1.0)
            gate, scale = rnd(1, C).tanh(), rnd(1, C, scale=0.3, shift=1.0)
            out, out_mod = torch.empty_like(res), torch.empty_like(res)
            for mode, (use_a, use_mod) in MODES.items():
                def kernel():
                    return sandwich_norm(res, a if use_a else None, w_post=w_post if use_a else None, gate=gate if use_a else None,
                                         w_pre=w_pre if use_mod else None, scale=scale if use_mod else None, out=out if use_a else False,
                                         out_mod=out_mod if use_mod else False)

                def torch_ops():
                    y = res + gate.unsqueeze(1) * rmsnorm(a, w_post) if use_a else res
                    return y, rmsnorm(y, w_pre) * scale.unsqueeze(1) if use_mod else None

                ko, km, _ = kernel()
                ty, tm = torch_ops()
                d_out = (ko.float() - ty.float()).abs().max().item() if use_a else 0.0
                d_mod = (km.float() - tm.float()).abs().max().item() if use_mod else 0.0
                t = alternate({"kernel": kernel, "torch": torch_ops}, args.repeats, args.inner)
                med = {k: statistics.median(xs) for k, xs in t.items()}
                tensors = 1 + int(use_a) + int(use_a) + int(use_mod)  # res, a read; out, out_mod written
                bound_ms = 2 * T * C * tensors / (COPY_TBS * 1e12) * 1e3
                emit(f"{dname}, T = {T}, mode {mode}: byte bound {bound_ms:.4f} ms; max |kernel - torch| out {d_out:.3g}, out_mod {d_mod:.3g}")
                emit(line("  svdq_sandwich_norm (1 launch)", t["kernel"],
                          f"  {bound_ms / med['kernel']:.2f} of the byte bound; kernel / torch = {med['kernel'] / med['torch']:.3f}"))
                emit(line("  torch ops (RMSNorm, gate, add, RMSNorm, scale)", t["torch"]))
            del res, a, out, out_mod


def bench_qk(args, emit, dev):
    from nunchaku_amd.ops import qk_norm_rope

    HD = H * 128
    emit("")
    emit(f"svdq_qk_norm_rope, H = {H} heads of 128, one sample, one launch per call (in place: every call normalises what the last one wrote; the "
         f"values stay finite); byte bound = Q, K, V read + Q, K, V^T written + freqs at {COPY_TBS} TB/s")
    g = torch.Generator(device=dev).manual_seed(1)
    for dname, dt in DTYPES.items():
        for T in TOKENS:
            L = (T + 127) // 128 * 128
            qkv0 = (2.0 * torch.randn(L, 3 * HD, device=dev, generator=g)).to(dt)
            wq, wk = (1 + 0.1 * torch.randn(128, device=dev, generator=g)).to(dt), (1 + 0.1 * torch.randn(128, device=dev, generator=g)).to(dt)
            ang = torch.rand(T, 64, device=dev, generator=g) * 6.2831853
            fc = torch.polar(torch.ones_like(ang), ang)
            vt = torch.empty(HD, L, dtype=dt, device=dev)
            qkv = qkv0.clone()

            def kernel():
                return qk_norm_rope(qkv, H, T, norm_q=wq, norm_k=wk, freqs_cis=fc, vt=vt)

            def torch_ops(src=qkv0):
                q, k, v = src[:T].unsqueeze(0).chunk(3, dim=-1)
                q, k = q.unflatten(-1, (H, -1)), k.unflatten(-1, (H, -1))
                q, k = rope(rmsnorm(q, wq), fc.unsqueeze(0)), rope(rmsnorm(k, wk), fc.unsqueeze(0))
                return q, k, v[0].t().contiguous()

            kernel()
            tq, tk, tv = torch_ops()
            dq = (qkv[:T, :HD].float() - tq.flatten(2)[0].float()).abs().max().item()
            dk = (qkv[:T, HD:2 * HD].float() - tk.flatten(2)[0].float()).abs().max().item()
            dv = (vt[:, :T].float() - tv.float()).abs().max().item()
            t = alternate({"kernel": kernel, "torch": torch_ops}, args.repeats, args.inner)
            med = {k: statistics.median(xs) for k, xs in t.items()}
            bound_ms = (2 * HD * (5 * T + L) + 8 * 64 * T) / (COPY_TBS * 1e12) * 1e3
            emit(f"{dname}, T = {T} (L_pad {L}): byte bound {bound_ms:.4f} ms; max |kernel - torch| Q {dq:.3g}, K {dk:.3g}, V^T {dv:.3g}")
            emit(line("  svdq_qk_norm_rope (1 launch)", t["kernel"],
                      f"  {bound_ms / med['kernel']:.2f} of the byte bound; kernel / torch = {med['kernel'] / med['torch']:.3f}"))
            emit(line("  torch ops (2 RMSNorm, 2 complex RoPE, V^T copy)", t["torch"]))
            del qkv0, qkv, vt


def torch_block(blk, x, fc, adaln):
    """the block as diffusers computes it in the 16-bit dtype, around the block's own SVDQW4A4Linear s"""
    scale_msa, gate_msa, scale_mlp, gate_mlp = blk.adaLN_modulation(adaln).unsqueeze(1).chunk(4, dim=-1)
    gate_msa, gate_mlp, scale_msa, scale_mlp = gate_msa.tanh(), gate_mlp.tanh(), 1.0 + scale_msa, 1.0 + scale_mlp
    at = blk.attention
    q, k, v = at.to_qkv(rmsnorm(x, blk.attention_norm1.weight) * scale_msa).chunk(3, dim=-1)
    q, k, v = (t.unflatten(-1, (at.heads, -1)) for t in (q, k, v))
    q, k = rope(rmsnorm(q, at.norm_q.weight), fc), rope(rmsnorm(k, at.norm_k.weight), fc)
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).flatten(2, 3)
    x = x + gate_msa * rmsnorm(at.to_out[0](o), blk.attention_norm2.weight)
    value, gate = blk.feed_forward.net[0].proj(rmsnorm(x, blk.ffn_norm1.weight) * scale_mlp).chunk(2, dim=-1)
    return x + gate_mlp * rmsnorm(blk.feed_forward.net[2](value * F.silu(gate)), blk.ffn_norm2.weight)


def bench_block(args, emit, dev):
    from nunchaku_amd.models.linear import SVDQW4A4Linear, synthetic_codes_
    from nunchaku_amd.models.zimage import NunchakuZImageTransformerBlock

    emit("")
    emit(f"a whole block, dim {C}, {H} heads, hidden {HIDDEN}, rank 32, random weights, B = 1: fused forward against the composition from 16-bit torch ops")
    g = torch.Generator(device=dev).manual_seed(2)
    inner = max(1, args.inner // 4)
    for dname, dt in DTYPES.items():
        blk = NunchakuZImageTransformerBlock(C, H, HIDDEN, rank=32, torch_dtype=dt, device=dev)
        with torch.no_grad():
            for m in blk.modules():
                if isinstance(m, SVDQW4A4Linear):
                    K = m.in_features
                    synthetic_codes_(m.qweight, m.wscales, K, g)
                    m.smooth_factor.copy_(torch.rand((K,), generator=g, device=dev) + 0.5)
                    m.smooth_factor_orig.copy_(m.smooth_factor)
                    m.proj_down.copy_(torch.randn(m.proj_down.shape, generator=g, device=dev) * 0.5 / math.sqrt(K))
                    m.proj_up.copy_(torch.randn(m.proj_up.shape, generator=g, device=dev) * 0.5 / math.sqrt(m.rank))
                elif isinstance(m, torch.nn.Linear):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g, device=dev) / math.sqrt(m.in_features))
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g, device=dev) * 0.1)
                elif isinstance(m, torch.nn.RMSNorm):
                    m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g, device=dev))
        for T in TOKENS:
            x = torch.randn(1, T, C, device=dev, generator=g).to(dt)
            ang = torch.rand(1, T, 64, device=dev, generator=g) * 6.2831853
            fc = torch.polar(torch.ones_like(ang), ang)
            adaln = torch.randn(1, 256, device=dev, generator=g).to(dt)
            with torch.no_grad():
                versions = {"fused": lambda: blk(x, None, fc, adaln), "torch": lambda: torch_block(blk, x, fc, adaln)}
                yf, yt = versions["fused"](), versions["torch"]()
                diff = (yf.float() - yt.float()).abs()
                t = alternate(versions, args.repeats, inner)
            med = {k: statistics.median(xs) for k, xs in t.items()}
            emit(f"{dname}, T = {T}: |fused - torch| max {diff.max().item():.3g}, mean {diff.mean().item():.3g} (max |y| {yt.float().abs().max().item():.3g}; "
                 "4-bit activations amplify a rounding flip of the glue)")
            emit(line("  block, fused (3 sandwich, 1 QK, svdq_attention)", t["fused"], f"  fused / torch = {med['fused'] / med['torch']:.3f}"))
            emit(line("  block, 16-bit torch ops around the linears", t["torch"]))
        del blk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-block", action="store_true")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_zimage: no GPU: nothing is measured without one")
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
    bench_sandwich(args, emit, dev)
    bench_qk(args, emit, dev)
    if not args.skip_block:
        bench_block(args, emit, dev)


if __name__ == "__main__":
    main()
