"""Record the calls the reference's own Python wrappers make into ``nunchaku._C.ops`` -> tests/golden/reference_shim_calls.json.

The reference's ``utils.py``, ``ops/*.py`` and ``models/linear.py`` are loaded by path, unmodified, behind a stub package
whose ``_C.ops`` records every call (operation name, positional and keyword arguments: tensors as shape + dtype, other
values as they are) and then raises, as the shim does on CPU tensors at the first launch.  Two callers are recorded:
``SVDQW4A4Linear.forward`` and ``fused_gelu_mlp`` on a [1, 4, 128] bf16 input, rank 16.  The fixture also keeps the
parameter shapes and dtypes of the reference's ``SVDQW4A4Linear(128, 256, rank=16)``.  tests/test_nunchaku_shim.py
replays the recorded calls against this repository's shim; the reference tree itself is not needed there.

    python tools/make_shim_calls.py PATH_TO_REFERENCE_CHECKOUT
"""

import importlib.util
import json
import os
import sys
import types

import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reference_shim_calls.json")


class _Stop(RuntimeError):
    pass


def _describe(v):
    if isinstance(v, torch.Tensor):
        return {"tensor": {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")}}
    if v is None or isinstance(v, (bool, int, float, str)):
        return {"value": v}
    raise TypeError(f"cannot record an argument of type {type(v).__name__}")


class _RecordingOps:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args, **kwargs):
            self.calls.append({"op": name, "args": [_describe(a) for a in args], "kwargs": {k: _describe(v) for k, v in kwargs.items()}})
            raise _Stop(name)
        return record


def _load_reference(ref_pkg: str, ops):
    def module(name, path=None):
        if path is None:
            m = types.ModuleType(name)
            m.__path__ = []
        else:
            spec = importlib.util.spec_from_file_location(name, path)
            m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        return m

    # the reference's ops/fused.py imports `nunchaku.models.linear` by absolute name: the stub package is called nunchaku
    module("nunchaku")
    c = module("nunchaku._C")
    c.ops = ops
    c.utils = types.SimpleNamespace()
    sys.modules["nunchaku"]._C = c
    module("nunchaku.ops")
    module("nunchaku.models")
    mods = {}
    for name, rel in ((".utils", "utils.py"), (".ops.quantize", "ops/quantize.py"), (".ops.gemm", "ops/gemm.py"), (".ops.gemv", "ops/gemv.py"),
                      (".models.linear", "models/linear.py"), (".ops.fused", "ops/fused.py")):
        m = module("nunchaku" + name, os.path.join(ref_pkg, rel))
        m.__spec__.loader.exec_module(m)
        mods[name] = m
    return mods


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_pkg = os.path.join(sys.argv[1], "nunchaku")
    ops = _RecordingOps()
    mods = _load_reference(ref_pkg, ops)
    RefLinear = mods[".models.linear"].SVDQW4A4Linear
    lin = RefLinear(128, 256, rank=16, torch_dtype=torch.bfloat16, device="cpu")
    x = torch.zeros(1, 4, 128, dtype=torch.bfloat16)
    callers = {}
    for caller, run in (("SVDQW4A4Linear.forward", lambda: lin(x)),
                        ("fused_gelu_mlp", lambda: mods[".ops.fused"].fused_gelu_mlp(
                            x, RefLinear(128, 256, rank=16, torch_dtype=torch.bfloat16, device="cpu"),
                            RefLinear(256, 128, rank=16, torch_dtype=torch.bfloat16, device="cpu")))):
        ops.calls = []
        try:
            run()
        except _Stop:
            pass
        assert len(ops.calls) == 1, f"{caller}: expected one recorded call, got {ops.calls}"
        callers[caller] = ops.calls[0]
    fixture = {
        "input": {"shape": list(x.shape), "dtype": "bfloat16"},
        "linear_128_256_r16": {k: _describe(v)["tensor"] for k, v in lin.state_dict().items()},
        "calls": callers,
    }
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in fixture.items()) + "\n}\n")
    print(f"wrote {os.path.relpath(OUT)}: {', '.join(k + ' -> ops.' + v['op'] for k, v in callers.items())}")


if __name__ == "__main__":
    main()
