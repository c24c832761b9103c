"""Timings of the Qwen-Image rotary-table build on one MI355X (bench.py stays the flagship benchmark and is not involved).

Two arms that produce the same five tables bit for bit (checked before anything is timed):
  torch ops   ``pack_qwen_rotary(*qwen_rope_freqs_multi(grids, L, device="cuda"))`` -- the torch-op sequence on the device, as the model ran
              it before ``svdq_qwen_rotary`` (for one grid: the sequence of ``qwen_rope_freqs``)
  one launch  ``ops.qwen_rotary`` from the model's axis tables; a third line times the launch that writes the joint table alone, which is
              what the fused path asks for
in two modes: eager calls, and replays of a captured graph that holds nothing but the build -- the case the kernel is for: a captured
Qwen-Image step builds its tables inside the graph on every replay.  Shapes: one grid (1, 64, 64) with 256 text tokens (a 1024 x 1024
image) and four such grids with 512 text tokens (an Edit step with three reference images).  The arms alternate inside one process,
event-bracketed, warm; min / median / max per arm.  The kernel nodes an arm puts into its graph are the kernels one call of it launches,
counted by the profiler.

    python tools/bench_qwen_rotary.py [--repeats 9] [--inner 20] [--out profiles/qwen_edit_rotary.txt]
"""

import argparse
import os
import re
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fbcache import alternate, line  # noqa: E402

SHAPES = (("one grid (1, 64, 64), 256 text tokens", [(1, 64, 64)], 256), ("four grids (1, 64, 64), 512 text tokens", [(1, 64, 64)] * 4, 512))


def captured(fn):
    """``fn`` captured alone into a graph (warm on the capture stream first) -> (replay, the captured outputs)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = fn()
    return graph.replay, out


def device_kernels(fn):
    """kernels one call of ``fn`` launches (each is one kernel node of a graph that captures the call), counted by the profiler; None where
    it records no device activity"""
    from torch.profiler import ProfilerActivity, profile

    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return len([n for n in names if not re.match(r"(?i)mem(cpy|set)", n)]) or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from nunchaku_amd import ops
    from nunchaku_amd.models.qwenimage import pack_qwen_rotary, qwen_rope_axis_tables, qwen_rope_freqs_multi

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; repeats {args.repeats} x inner {args.inner}, arms alternated; ms per build"]
    pos_cs, neg_cs = qwen_rope_axis_tables(device=dev)
    for name, grids, L in SHAPES:
        arms = {
            "torch ops (five tables)": lambda: pack_qwen_rotary(*qwen_rope_freqs_multi(grids, L, device=dev)),
            "one launch (five tables)": lambda: ops.qwen_rotary(pos_cs, neg_cs, grids, L),
            "one launch (joint table alone)": lambda: ops.qwen_rotary(pos_cs, neg_cs, grids, L, tables=("all",)),
        }
        ref, got = arms["torch ops (five tables)"](), arms["one launch (five tables)"]()
        assert all(torch.equal(ref[k].view(torch.int32), got[k].view(torch.int32)) for k in ref), "the arms differ"
        written = sum(t.numel() * 4 for t in got.values())
        lines.append(f"{name}: {sum(f * h * w for f, h, w in grids)} image rows, {written / 1e6:.2f} MB of tables (all five), arms bit-equal")
        t = alternate(arms, args.repeats, args.inner)
        lines.append("  eager calls")
        for k in arms:
            lines.append(line("    " + k, t[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"    one launch / torch ops (medians, five tables): {med['one launch (five tables)'] / med['torch ops (five tables)']:.3f}; "
                     f"the launch writes {written / 1e6 / med['one launch (five tables)']:.1f} GB/s")
        replays, counts = {}, {}
        for k, fn in arms.items():
            counts[k] = device_kernels(fn)
            replays[k], out = captured(fn)
            replays[k]()
            torch.cuda.synchronize()
            assert all(torch.equal(out[n].view(torch.int32), ref[n].view(torch.int32)) for n in out), f"{k}: the graph's tables differ"
        t = alternate(replays, args.repeats, args.inner)
        lines.append("  replays of a graph that holds the build alone")
        for k in arms:
            nodes = "not counted" if counts[k] is None else str(counts[k])
            lines.append(line("    " + k, t[k], f"  kernel nodes: {nodes}"))
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"    one launch / torch ops (medians, five tables): {med['one launch (five tables)'] / med['torch ops (five tables)']:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
