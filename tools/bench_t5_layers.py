"""Timings of the fused T5 encoder layer pieces on one MI355X (bench.py stays the flagship benchmark and is not involved), bf16:

* QKV:  one ``gemm_awq_multi`` CONCAT launch against three ``gemm_awq`` launches, K = 4096, Ns = (4096, 4096, 4096), M = 8 / 256 / 512;
* FF:   the GATED launch against two ``gemm_awq`` + transformers' ``NewGELUActivation`` + the product, N = 10240, the same M;
* norm: ``t5_residual_norm`` (add + norm, one pass) against the torch add + ``T5LayerNorm`` at 512 x 4096;
* the 24-layer T5-XXL-shaped encoder (random 4-bit weights, B = 1) at 256 and 512 tokens with ``set_fused_layers`` on and off, as eager calls
  and as captured replays.

Arms alternate inside one process, the whole round repeated: min / median / max per arm between device events, with the median shader clock.

    python tools/bench_t5_layers.py [--repeats 7] [--inner 20] [--no-encoder] [--out profiles/t5_fused_layers.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_awq_gemm import Clock  # noqa: E402
from tools.bench_sdxl_attention import alternate, line  # noqa: E402

D, F = 4096, 10240


def random_w4(lin):
    """fill a W4Linear's buffers with random codes and plausible scales (no quantisation pass: the timings do not depend on the values)"""
    lin.qweight.copy_(torch.randint(-2 ** 15, 2 ** 15, lin.qweight.shape, device=lin.qweight.device, dtype=torch.int16))
    lin.scales.copy_(torch.rand_like(lin.scales.float()) * 0.002 + 0.001)
    lin.scaled_zeros.copy_(-7.5 * lin.scales.float())
    return lin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-encoder", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import transformers
    from transformers.activations import NewGELUActivation
    from transformers.models.t5.modeling_t5 import T5LayerNorm

    from nunchaku_amd._C import ops
    from nunchaku_amd.models.text_encoders import W4Linear
    from nunchaku_amd.models.text_encoders.t5_encoder import ATTENTION_NAME, register_fused_attention, set_fused_layers
    from nunchaku_amd.ops import gemm_awq_multi, t5_residual_norm

    if not torch.cuda.is_available():
        raise SystemExit("bench_t5_layers: no GPU: a timing needs the MI355X (nothing is measured on the CPU)")
    torch.cuda.set_device(0)
    clock, lines, dt = Clock(), [], torch.bfloat16

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def arms(title, versions, graph):
        clock.mark()
        res = alternate(versions, args.repeats, args.inner, graph=graph)
        emit(f"{title}  [{'captured replays' if graph else 'eager calls'}; median shader clock {clock.mark()} GHz]")
        for k, xs in res.items():
            emit("  " + line(k, xs))

    emit(f"# tools/bench_t5_layers.py --repeats {args.repeats} --inner {args.inner}: ms per call, arms alternated, bf16")
    torch.manual_seed(0)
    mk = lambda k, n: random_w4(W4Linear(k, n, group_size=128, dtype=dt, device="cuda"))
    q, k, v, wi0, wi1 = mk(D, D), mk(D, D), mk(D, D), mk(D, F), mk(D, F)
    one = lambda x, l: ops.gemm_awq(x, l.qweight, l.scales, l.scaled_zeros)
    act = NewGELUActivation()
    for M in (8, 256, 512):
        x = torch.randn(M, D, device="cuda").to(dt)
        arms(f"QKV M={M} K={D} Ns=3x{D}", {"gemm_awq_multi concat (1 launch)": lambda: gemm_awq_multi(x, (q, k, v)),
                                         "3 x gemm_awq": lambda: (one(x, q), one(x, k), one(x, v))}, True)
        arms(f"FF  M={M} K={D} N={F}", {"gemm_awq_multi gated_gelu_new (1 launch)": lambda: gemm_awq_multi(x, (wi0, wi1), "gated_gelu_new"),
                                       "2 x gemm_awq + NewGELUActivation + mul": lambda: act(one(x, wi0)) * one(x, wi1)}, True)
    norm = T5LayerNorm(D).to("cuda", dt)
    res, a = torch.randn(512, D, device="cuda").to(dt), torch.randn(512, D, device="cuda").to(dt)

    def torch_norm():
        y = res + a
        return y, norm(y)

    with torch.no_grad():
        arms(f"norm 512 x {D}: add + T5LayerNorm", {"t5_residual_norm (1 launch)": lambda: t5_residual_norm(res, a, norm.weight.data, 1e-6),
                                                   "torch add + T5LayerNorm": torch_norm}, True)
    if args.no_encoder:
        return
    cfg = transformers.T5Config(vocab_size=32128, d_model=D, d_kv=64, d_ff=F, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu",
                                dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    with torch.device("meta"):
        model = transformers.T5EncoderModel(cfg).to(dt).eval()
    for mod in list(model.modules()):
        for cname, child in list(mod.named_children()):
            if isinstance(child, torch.nn.Linear):
                setattr(mod, cname, W4Linear.from_linear(child, group_size=128, init_only=True))
    model.to_empty(device="cuda")
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, W4Linear):
                random_w4(mod)
                mod.weight = torch.empty(0, dtype=dt, device="meta")
            elif isinstance(mod, T5LayerNorm):
                mod.weight.fill_(1.0)
            elif isinstance(mod, torch.nn.Embedding):
                mod.weight.normal_()
    if register_fused_attention():
        model.config._attn_implementation = ATTENTION_NAME
    ids = {T: torch.randint(0, 32128, (1, T), device="cuda") for T in (256, 512)}

    def run(flag, T):
        set_fused_layers(model, flag)
        return model(input_ids=ids[T]).last_hidden_state

    with torch.no_grad():
        for graph in (False, True):  # (the captured arms last: a capture that fails ends the run, with the eager figures written)
            for T in ids:
                if not graph:
                    cos = torch.nn.functional.cosine_similarity(run(True, T)[0].float(), run(False, T)[0].float(), dim=-1)
                    emit(f"encoder 24 layers, {T} tokens: token cosine fused vs parent path min {cos.min().item():.5f} mean {cos.mean().item():.5f}")
                try:
                    arms(f"encoder 24 layers, B=1, T={T}", {"fused_layers=True": lambda: run(True, T),
                                                           "fused_layers=False (parent path)": lambda: run(False, T)}, graph)
                except RuntimeError as e:
                    emit(f"encoder 24 layers, B=1, T={T} [captured replays]: NOT MEASURED, the capture failed: {str(e).splitlines()[0]}")
                    return


if __name__ == "__main__":
    main()
