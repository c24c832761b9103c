"""Timings of SANA's block glue and of a whole SANA block on one MI355X (bench.py stays the flagship benchmark and is not involved).

Part 1, the kernel: ``svdq_sana_glue`` (one launch; bf16) at SANA-1.6B's 2240 channels in 2304-wide rows and SANA-0.6B's 1152, T in {1024, 4096,
16384} tokens, B in {2, 3}, in the three modes a block runs it in --

  msa    out = a * gate_msa + res                                                          (reads a, res; writes out)
  cross  out = a + res;  out_mod = LayerNorm(out) * (scale_mlp + 1) + shift_mlp            (reads a, res; writes out, out_mod)
  mlp    out = a * gate_mlp + res;  out_mod = LayerNorm(out) * (scale_msa' + 1) + shift_msa'  with the next block's table

-- against

  (a) the 16-bit torch-op sequence it replaces: the add of the table to timestep (the modes that read a table), multiply-add, ``layer_norm``,
      multiply-add and the ``F.pad`` to the GEMM operand width of what is handed on (nothing to pad at 1152);
  (b) its byte bound: the 16-bit elements it must read (a, res: C each) and write (C_pad per output) at the chip's measured copy figure.
      The tables and timestep (12 * C * (B + 1) bytes) are left out of the bound.

Outputs of the kernel and of (a) are compared at every size before anything is timed (torch's layer_norm forms its statistics in another
order: the last 16-bit place may differ).

Part 2, a block: ``SanaLinearTransformerBlock.forward_padded`` with random weights for SANA-1.6B and SANA-0.6B at 32 x 32 and 64 x 64 tokens,
B = 2, 300 text tokens per sample, and its parts on the same inputs: the three layers and the four glue launches of a block run alone (inside
the stack a block has three).  The parts are timed one at a time; their sum is not the block's time (launch gaps, cache state) and both are shown.

Event-bracketed, warm; the versions alternate inside one process and the whole round is repeated: min / median / max per version.

    python tools/bench_sana_block.py [--repeats 7] [--inner 20] [--out profiles/sana_block.txt] [--skip-block]
"""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

COPY_TBS = 6.29  # float4 copy on MI355X
WIDTHS = [(2240, 2304), (1152, 1152)]
TOKENS = [1024, 4096, 16384]
MODELS = {"SANA-1.6B": (2240, 20), "SANA-0.6B": (1152, 16)}
MODES = {  # name -> (gate row, (shift, scale) rows of out_mod or None)
    "msa": (2, None),
    "cross": (None, (3, 4)),
    "mlp": (5, (0, 1)),
}


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


def glue_bytes(mode: str, rows: int, C: int, C_pad: int) -> int:
    """what the pass must move: a and res read, one or two C_pad-wide outputs written, 2 bytes each"""
    outputs = 1 if MODES[mode][1] is None else 2
    return 2 * rows * (2 * C + outputs * C_pad)


def bench_kernel(args, emit, dev):
    from nunchaku_amd.ops import sana_glue

    emit(f"svdq_sana_glue, bf16, one launch per call; byte bound = 2 * B * T * (2 * C + outputs * C_pad) bytes at {COPY_TBS} TB/s; no counter run was made")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, device=dev, generator=g)).bfloat16()
    for C, C_pad in WIDTHS:
        for T in TOKENS:
            for B in args.batches:
                res, a_wide = rnd(B, T, C_pad), rnd(B, T, C_pad)
                res[..., C:] = 0
                a = a_wide[..., :C]
                ts, tab, nxt = rnd(B, 6, C, scale=0.5), rnd(6, C, scale=0.5), rnd(6, C, scale=0.5)
                out, out_mod = torch.empty(B, T, C_pad, device=dev, dtype=torch.bfloat16), torch.empty(B, T, C_pad, device=dev, dtype=torch.bfloat16)
                for mode, (gate_row, mod_rows) in MODES.items():
                    mtab = nxt if mode == "mlp" else tab

                    def kernel():
                        return sana_glue(res, a, timestep=ts, gate_table=tab if gate_row is not None else None, gate_row=gate_row,
                                         mod_table=mtab if mod_rows else None, scale_row=mod_rows[1] if mod_rows else None,
                                         shift_row=mod_rows[0] if mod_rows else None, channels=C, pad_to=C_pad, out=out,
                                         out_mod=out_mod if mod_rows else False)

                    def torch_ops():
                        h = a
                        if gate_row is not None:
                            h = h * (ts + tab[None])[:, gate_row:gate_row + 1]
                        h = h + res[..., :C]
                        m = None
                        if mod_rows:
                            mod = ts + mtab[None]
                            m = F.layer_norm(h, (C,), eps=1e-6) * (mod[:, mod_rows[1]:mod_rows[1] + 1] + 1) + mod[:, mod_rows[0]:mod_rows[0] + 1]
                        if C_pad != C:
                            h = F.pad(h, (0, C_pad - C))
                            m = None if m is None else F.pad(m, (0, C_pad - C))
                        return h, m

                    ko, km, _ = kernel()
                    th, tm = torch_ops()
                    diff = (ko.float() - th.float()).abs().max().item()
                    dmod = (km.float() - tm.float()).abs().max().item() if mod_rows else 0.0
                    t = alternate({"kernel": kernel, "torch": torch_ops}, args.repeats, args.inner)
                    med = {k: statistics.median(xs) for k, xs in t.items()}
                    bound_ms = glue_bytes(mode, B * T, C, C_pad) / (COPY_TBS * 1e12) * 1e3
                    emit(f"C = {C} in {C_pad}, T = {T}, B = {B}, mode {mode}: byte bound {bound_ms:.4f} ms; max |kernel - torch| out {diff:.3g}, out_mod {dmod:.3g}")
                    emit(line("  svdq_sana_glue (1 launch)", t["kernel"],
                              f"  {bound_ms / med['kernel']:.2f} of the byte bound; kernel / torch = {med['kernel'] / med['torch']:.3f}"))
                    emit(line("  torch ops (add, mul-add, layer_norm, pad)", t["torch"]))
                del res, a_wide, out, out_mod


def bench_block(args, emit, dev):
    from nunchaku_amd.models import SanaLinearTransformerBlock, sana_intermediate_size
    from nunchaku_amd.ops import sana_glue

    emit("")
    emit("a whole block, bf16, random weights, B = 2, 300 text tokens per sample (padded form); parts timed alone on the block's own inputs")
    g = torch.Generator(device=dev).manual_seed(1)
    B, L = 2, 300
    for name, (dim, cross_heads) in MODELS.items():
        block = SanaLinearTransformerBlock(dim, sana_intermediate_size(dim, 2.5), cross_heads, device=dev)
        with torch.no_grad():
            for p in block.parameters():
                if p.dtype in (torch.int8, torch.int32):
                    p.copy_(torch.randint(-100, 100, p.shape, device=dev, generator=g).to(p.dtype))
                else:
                    p.copy_(torch.randn(p.shape, device=dev, generator=g) * (0.5 if p.dim() == 1 else 0.02))
        dp = block.dim_pad
        for side in (32, 64):
            T = side * side
            x = torch.randn(B, T, dim, device=dev, generator=g).bfloat16()
            ts = (0.5 * torch.randn(B, 6 * dim, device=dev, generator=g)).bfloat16()
            cond = torch.randn(B, L, dim, device=dev, generator=g).bfloat16()
            kc = torch.full((B,), L, dtype=torch.int32, device=dev)
            t3 = ts.view(B, 6, dim)
            h, hm = block.modulate_msa(x, t3)
            a = block.attn(hm)
            tab = block.scale_shift_table
            glue = dict(timestep=t3, channels=dim, pad_to=dp)
            o, om = torch.empty(B, T, dp, device=dev, dtype=torch.bfloat16), torch.empty(B, T, dp, device=dev, dtype=torch.bfloat16)
            parts = {
                "block.forward_padded": lambda: block.forward_padded(x, cond, ts, kc, side, side),
                "attn (qkv, linear attention, out)": lambda: block.attn(hm),
                "cross_attn (q, kv, attention, out)": lambda: block.cross_attn.forward_padded(h, cond, kc),
                "ff (inverted, depthwise, point)": lambda: block.ff(hm, side, side),
                "glue: first modulate": lambda: block.modulate_msa(x, t3),
                "glue: msa": lambda: sana_glue(h, a, gate_table=tab, gate_row=2, out=o, out_mod=False, **glue),
                "glue: cross": lambda: sana_glue(h, a, mod_table=tab, scale_row=4, shift_row=3, out=o, out_mod=om, **glue),
                "glue: mlp": lambda: sana_glue(h, a, gate_table=tab, gate_row=5, mod_table=tab, scale_row=1, shift_row=0, out=o, out_mod=om, **glue),
            }
            t = alternate(parts, args.repeats, args.inner)
            med = {k: statistics.median(xs) for k, xs in t.items()}
            total = sum(v for k, v in med.items() if k != "block.forward_padded")
            emit(f"{name}: dim {dim} in {dp}, {side} x {side} = {T} tokens, B = {B}: block {med['block.forward_padded']:.4f} ms, sum of its parts {total:.4f} ms")
            for k, xs in t.items():
                share = "" if k == "block.forward_padded" else f"  {100 * med[k] / total:5.1f} % of the sum"
                emit(line("  " + k, xs, share))
            glue_ms = sum(v for k, v in med.items() if k.startswith("glue"))
            emit(f"  glue, four launches: {glue_ms:.4f} ms = {100 * glue_ms / total:.1f} % of the sum")
        del block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=(2, 3))
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-block", action="store_true")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_sana_block: no GPU: nothing is measured without one")
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
    bench_kernel(args, emit, dev)
    if not args.skip_block:
        bench_block(args, emit, dev)


if __name__ == "__main__":
    main()
