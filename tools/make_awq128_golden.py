"""Generate tests/golden/awq128_*.npz and tests/golden/awq128_w4linear_spec.json from the REFERENCE's own tinychat
converter and W4Linear (run in the build container only; the reference does not exist on the GPU box).

`nunchaku/models/text_encoders/tinychat_utils.py` is pure torch and is loaded by path; `linear.py` is loaded behind stub
parent packages whose `_C.ops` is empty (only the constructor runs).  Each .npz holds the logical quantised layer --
codes [N, K] (uint8; the converter's input weight is bf16(codes * scale - zero) in fp32), per-group scale and zero (fp32 holding bf16 values, zero in code units times scale) -- and the
converter's packed `qweight` (int16 [N/4, K]), `scales` / `scaled_zeros` (bf16 bits as uint16, [ceil_num_groups, N]).
Group 128; K = 640 has 5 groups padded to 8, so the padding rows are pinned.

    python tools/make_awq128_golden.py PATH_TO_REFERENCE_CHECKOUT
"""

import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for pkg in ("nunchaku", "nunchaku.models", "nunchaku.models.text_encoders"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    c = types.ModuleType("nunchaku._C")
    c.ops = types.SimpleNamespace(gemm_awq=None, gemv_awq=None)
    sys.modules["nunchaku._C"] = c
    sys.modules["nunchaku._C.ops"] = c.ops
    tu = _load("nunchaku.models.text_encoders.tinychat_utils", f"{REF}/nunchaku/models/text_encoders/tinychat_utils.py")
    lin = _load("nunchaku.models.text_encoders.linear", f"{REF}/nunchaku/models/text_encoders/linear.py")
    return tu, lin


def main():
    if not REF:
        sys.exit("usage: python tools/make_awq128_golden.py PATH_TO_REFERENCE_CHECKOUT")
    os.makedirs(OUT, exist_ok=True)
    tu, lin = load_reference()
    rng = np.random.default_rng(20261016)
    for (N, K) in ((64, 640), (256, 1024)):
        G = K // 128
        codes = rng.integers(0, 16, size=(N, K), dtype=np.int64)
        scale = torch.tensor(rng.uniform(0.002, 0.05, size=(N, G)), dtype=torch.float32).bfloat16()
        zero = (torch.tensor(rng.integers(0, 16, size=(N, G)), dtype=torch.float32) * scale.float()).bfloat16()
        # weight on the grid: (q * s - z) in fp32, rounded to bf16 (what W4Linear.from_linear hands the converter; the tests rebuild it the same way)
        w = (torch.tensor(codes, dtype=torch.float32).view(N, G, 128) * scale.float().view(N, G, 1) - zero.float().view(N, G, 1)).view(N, K).bfloat16()
        qw, sc, zr = tu.convert_to_tinychat_w4x16y16_linear_weight(w, scale, zero, group_size=128)
        # the converter derives the codes back from w: the bf16 rounding of w moves them by < 15 * 2^-9 of a step
        q_conv = torch.round((w.float().view(N, G, 128) + zero.float().view(N, G, 1)) / scale.float().view(N, G, 1)).view(N, K)
        assert torch.equal(q_conv, torch.tensor(codes, dtype=torch.float32))
        np.savez_compressed(os.path.join(OUT, f"awq128_{N}x{K}.npz"),
                            codes=codes.astype(np.uint8),
                            scale=scale.float().numpy(), zero=zero.float().numpy(),
                            qweight=qw.numpy(), scales=sc.view(torch.int16).numpy().view(np.uint16),
                            scaled_zeros=zr.view(torch.int16).numpy().view(np.uint16),
                            ceil_num_groups=np.int64(tu.ceil_num_groups(K, 128, 4)))
        print(f"awq128_{N}x{K}.npz: qweight {tuple(qw.shape)} scales {tuple(sc.shape)}")
    table = [[k, g, tu.ceil_num_groups(k, g, 4)] for k in (128, 256, 640, 1024, 1536, 4096, 10240, 3072, 64 * 5, 32 * 7)
             for g in (32, 64, 128, 256) if k % g == 0]
    spec = {}
    for bias in (False, True):
        m = lin.W4Linear(640, 256, bias=bias, group_size=128, dtype=torch.bfloat16, device="cpu")
        spec[f"bias={bias}"] = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
    with open(os.path.join(OUT, "awq128_w4linear_spec.json"), "w") as f:
        json.dump({"W4Linear(640, 256, group_size=128, dtype=bfloat16)": spec, "ceil_num_groups": table}, f, indent=1)
    print("awq128_w4linear_spec.json")


if __name__ == "__main__":
    main()
