"""Time of the AWQ GEMV low-rank launch (svdq_gemv_awq_lora_batched) for a full FLUX.1-dev step's modulation layers -- 19 x 2 projections
3072 -> 18432 and 38 projections 3072 -> 9216, LoRA rank 16 and 64, bf16 -- against the same update as two torch.matmul per layer (device
events, five windows each; needs a GPU)."""
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nunchaku_amd._C import ops

dev, dt, K = "cuda", torch.bfloat16, 3072
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(K, device=dev, generator=g).to(dt)
Ns = [18432] * 38 + [9216] * 38


def timed(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps * 1e3)
    return ts


for r in (16, 64):
    entries, dense = [], []
    for i, N in enumerate(Ns):
        lo = SimpleNamespace(down=(torch.randn(r, K, device=dev, generator=g) / K ** 0.5).to(dt), up=(torch.randn(N, r, device=dev, generator=g) * 0.1).to(dt),
                             t=torch.zeros(r, device=dev, dtype=dt), strength=1e-3)
        out = torch.randn(N, device=dev, generator=g).to(dt)
        entries.append((lo, out, 6 if i < 38 else 3))
        dense.append((lo.down, lo.up, out.clone()))

    def new():
        ops.gemv_awq_lora_batched(x, entries)

    def mm():
        for down, up, out in dense:
            out.add_(torch.matmul(up, torch.matmul(down, x)), alpha=1e-3)

    tn, tm = timed(new), timed(mm, reps=50)
    mb = sum(r * K * 2 + N * r * 2 + 4 * N for N in Ns) / 1e6
    print(f"r={r}: 76 entries, {mb:.1f} MB touched | svdq_gemv_awq_lora_batched (2 launches): {min(tn):.1f} us (5 windows: {' '.join(f'{t:.1f}' for t in tn)}) "
          f"= {mb / min(tn) * 1e-3:.2f} TB/s | 2 torch.matmul + add per layer (228 launches): {min(tm):.1f} us (5 windows: {' '.join(f'{t:.1f}' for t in tm)})", flush=True)
