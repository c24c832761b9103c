"""Time the AWQ W4A16 GEMM (ops.gemm_awq, group 128) against hipBLASLt's dense bf16 GEMM (torch.nn.functional.linear on the
dequantised weights) at the seven projections of a T5-XXL encoder block, and the whole 24-layer encoder (512 tokens, random
weights) against the dense bf16 T5EncoderModel.  One process, same inputs, arms alternated, warmed up, device events.

    python tools/bench_awq_gemm.py [--kernels-only] [--iters 50]

--kernels-only: the GEMM launches alone (for a rocprofv3 --kernel-trace --stats run of its own).  Prints one JSON line per row.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nunchaku_amd._C import ops  # noqa: E402
from nunchaku_amd.models.text_encoders import W4Linear  # noqa: E402
from tests.test_awq_gemm_host import dequantise  # noqa: E402

PEAK_BF16 = 2.5e15  # dense bf16 MFMA peak of the MI355X, FLOP/s
HBM = 6.3e12  # measured streaming bandwidth, B/s
D, F = 4096, 10240
PROJ = [("q", D, D), ("k", D, D), ("v", D, D), ("o", D, D), ("wi_0", D, F), ("wi_1", D, F), ("wo", F, D)]  # (name, K, N)


class Clock:
    """median shader clock (GHz) over a region: the `*` line of the card's pp_dpm_sclk, read every 50 ms by a thread (bench.py's ClockSampler)"""

    def __init__(self):
        import glob
        import threading

        self.path, self.samples, self.stop_ev = None, [], threading.Event()
        try:
            pr = torch.cuda.get_device_properties(0)
            bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            for f in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
                if os.path.basename(os.path.realpath(os.path.dirname(f))).lower() == bdf:
                    self.path = f
        except Exception:
            pass
        if self.path:
            threading.Thread(target=self._run, daemon=True).start()

    def _run(self):
        import re

        while not self.stop_ev.is_set():
            try:
                m = re.search(r"(\d+)Mhz\s*\*", open(self.path).read())
                if m:
                    self.samples.append(int(m.group(1)))
            except Exception:
                pass
            self.stop_ev.wait(0.05)

    def mark(self):
        xs, self.samples = sorted(self.samples), []
        return xs[len(xs) // 2] / 1e3 if len(xs) >= 3 else None


CLOCK = None


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def layers():
    out = []
    for name, K, N in PROJ:
        lin = torch.nn.Linear(K, N, bias=False, device="cuda", dtype=torch.bfloat16)
        torch.nn.init.normal_(lin.weight, std=K ** -0.5)
        q = W4Linear.from_linear(lin, group_size=128)
        w16 = dequantise(q.qweight, q.scales, q.scaled_zeros, K)
        out.append((name, K, N, q, w16))
    return out


def bench_block(iters, kernels_only):
    ls = layers()
    rows = []
    for M in (8, 512, 1024):
        xs = {K: torch.randn(M, K, device="cuda").bfloat16() for K in (D, F)}
        awq = lambda: [ops.gemm_awq(xs[K], q.qweight, q.scales, q.scaled_zeros) for _, K, N, q, w in ls]  # noqa: E731
        dense = lambda: [torch.nn.functional.linear(xs[K], w) for _, K, N, q, w in ls]  # noqa: E731
        for _ in range(5):
            awq(); dense()
        torch.cuda.synchronize()
        if kernels_only:
            for _ in range(iters):
                awq()
            torch.cuda.synchronize()
            continue
        ta, td = [], []
        CLOCK.mark()
        for _ in range(5):  # alternate the arms
            ta.append(timed(awq, iters // 5))
            td.append(timed(dense, iters // 5))
        t_awq, t_dense = min(ta), min(td)
        flops = sum(2.0 * M * K * N for _, K, N, _, _ in ls)
        bytes_awq = sum(N * K / 2 + 4 * (K // 128) * N + 2 * M * (K + N) for _, K, N, _, _ in ls)
        bytes_dense = sum(2 * N * K + 2 * M * (K + N) for _, K, N, _, _ in ls)
        row = {"M": M, "block_awq_ms": round(t_awq, 4), "block_dense_bf16_ms": round(t_dense, 4), "awq_over_dense": round(t_awq / t_dense, 3),
               "awq_share_of_bf16_peak": round(flops / (t_awq * 1e-3) / PEAK_BF16, 3), "dense_share_of_bf16_peak": round(flops / (t_dense * 1e-3) / PEAK_BF16, 3),
               "awq_TBps": round(bytes_awq / (t_awq * 1e-3) / 1e12, 2), "awq_share_of_hbm": round(bytes_awq / (t_awq * 1e-3) / HBM, 3),
               "dense_TBps": round(bytes_dense / (t_dense * 1e-3) / 1e12, 2), "GFLOP": round(flops / 1e9, 1),
               "awq_spread_ms": [round(min(ta), 4), round(max(ta), 4)], "dense_spread_ms": [round(min(td), 4), round(max(td), 4)],
               "shader_clock_ghz": CLOCK.mark()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_encoder(iters):
    import transformers

    cfg = transformers.T5Config(vocab_size=32128, d_model=D, d_kv=64, d_ff=F, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu",
                                dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    with torch.device("cuda"):
        dense = transformers.T5EncoderModel(cfg).bfloat16().eval()
    quant = {}
    with torch.no_grad():
        for name, mod in list(dense.named_modules()):
            for cname, child in list(mod.named_children()):
                if isinstance(child, torch.nn.Linear):
                    torch.nn.init.normal_(child.weight, std=child.in_features ** -0.5)
                    q = W4Linear.from_linear(child, group_size=128)
                    child.weight.copy_(dequantise(q.qweight, q.scales, q.scaled_zeros, child.in_features))
                    quant[(mod, cname)] = (q, child)

    def use(which):
        for (mod, cname), (q, d) in quant.items():
            setattr(mod, cname, q if which == "awq" else d)

    ids = torch.randint(0, 32128, (1, 512), device="cuda")
    fwd = lambda: dense(input_ids=ids).last_hidden_state  # noqa: E731
    res = {}
    CLOCK.mark()
    with torch.no_grad():
        for which in ("awq", "dense", "awq", "dense"):
            use(which)
            for _ in range(3):
                fwd()
            t = timed(fwd, iters)
            res[which] = min(res.get(which, 1e9), t)
        use("awq")
        a = fwd().float()
        use("dense")
        b = fwd().float()
    clk = CLOCK.mark()
    cos = torch.nn.functional.cosine_similarity(a.flatten(0, 1), b.flatten(0, 1), dim=-1)
    row = {"encoder_24_layers_512_tokens_awq_ms": round(res["awq"], 3), "encoder_dense_bf16_ms": round(res["dense"], 3),
           "awq_over_dense": round(res["awq"] / res["dense"], 3), "token_cosine_awq_vs_dense_min_mean": [round(cos.min().item(), 5), round(cos.mean().item(), 5)], "shader_clock_ghz": clk,
           "weight_bytes_awq_linears": sum(q.qweight.numel() * 2 + q.scales.numel() * 4 for q, _ in quant.values()),
           "weight_bytes_dense_linears": sum(d.weight.numel() * 2 for _, d in quant.values())}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_awq_gemm needs a GPU"
    global CLOCK
    CLOCK = Clock()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count}), flush=True)
    bench_block(a.iters, a.kernels_only)
    if not a.kernels_only and not a.no_encoder:
        bench_encoder(max(5, a.iters // 5))


if __name__ == "__main__":
    main()
