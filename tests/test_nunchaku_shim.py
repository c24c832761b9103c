"""The ``nunchaku`` import surface: the reference's package layout resolves to the MI355X
implementation, and the calls the reference's OWN, UNMODIFIED ``ops/*.py`` and ``models/linear.py`` make into ``nunchaku._C``
(recorded once from those files: tests/golden/reference_shim_calls.json) run against the shim up to the first kernel launch
(which needs a GPU: the call must arrive in this library with the reference's positional arguments)."""
import json
import os

import pytest
import torch


def test_reference_import_paths_resolve():
    import nunchaku
    from nunchaku import NunchakuFluxTransformer2DModelV2, NunchakuFluxTransformer2dModel, NunchakuQwenImageTransformer2DModel
    from nunchaku._C import ops, utils
    from nunchaku.models.linear import AWQW4A16Linear, SVDQW4A4Linear
    from nunchaku.models.transformers.transformer_flux_v2 import NunchakuFluxTransformer2DModelV2 as V2
    from nunchaku.models.utils import CPUOffloadManager
    from nunchaku.ops.fused import fused_gelu_mlp, fused_qkv_norm_rottary
    from nunchaku.ops.gemm import svdq_gemm_w4a4_cuda
    from nunchaku.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda
    from nunchaku.utils import ceil_divide, get_precision

    assert V2 is NunchakuFluxTransformer2DModelV2 and NunchakuFluxTransformer2dModel is V2
    for name in ("gemm_w4a4", "quantize_w4a4_act_fuse_lora", "attention_fp16", "gemv_awq"):
        assert callable(getattr(ops, name)), name
    for name in ("set_log_level", "disable_memory_auto_release", "trim_memory", "set_faster_i2f_mode"):
        assert getattr(utils, name)("x") is None if name in ("set_log_level", "set_faster_i2f_mode") else getattr(utils, name)() is None
    assert get_precision() == "int4" and ceil_divide(5, 2) == 3
    lin = SVDQW4A4Linear(128, 256, rank=16, device="cpu")
    assert tuple(lin.qweight.shape) == (256, 64) and lin.qweight.dtype == torch.int8
    assert all(callable(f) for f in (fused_gelu_mlp, fused_qkv_norm_rottary, svdq_gemm_w4a4_cuda, svdq_quantize_w4a4_act_fuse_lora_cuda))
    assert CPUOffloadManager.__name__ == "CPUOffloadManager" and AWQW4A16Linear and NunchakuQwenImageTransformer2DModel and nunchaku.__all__


def _make(desc):
    if "tensor" in desc:
        return torch.zeros(desc["tensor"]["shape"], dtype=getattr(torch, desc["tensor"]["dtype"]))
    return desc["value"]


def test_unmodified_reference_callers_bind_to_the_shim(golden_dir):
    """The calls the reference's own ``ops/*.py`` and ``models/linear.py`` make into ``_C.ops`` (recorded from the unmodified files by
    tools/make_shim_calls.py -> tests/golden/reference_shim_calls.json) arrive in this library with the reference's positional arguments."""
    from nunchaku import _C
    from nunchaku.models.linear import SVDQW4A4Linear

    rec = json.load(open(os.path.join(golden_dir, "reference_shim_calls.json")))
    # the reference's SVDQW4A4Linear(128, 256, rank=16) holds the same parameters as ours
    assert tuple(rec["linear_128_256_r16"]["qweight"]["shape"]) == (256, 64)
    ours = SVDQW4A4Linear(128, 256, rank=16, torch_dtype=torch.bfloat16, device="cpu").state_dict()
    assert {k: {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")} for k, v in ours.items()} == rec["linear_128_256_r16"]
    # the reference's forward -> its quantize() -> its ops/quantize.py wrapper (allocates the [M_pad, K/2] buffer) -> shim
    # _C.ops.quantize_w4a4_act_fuse_lora with the reference's 8 positional arguments: arrives in this library, which has no
    # CPU path and says so (on a GPU the same call runs: tests/test_gpu_parity.py::test_reference_style_calls...); the same for fused_gelu_mlp
    assert set(rec["calls"]) == {"SVDQW4A4Linear.forward", "fused_gelu_mlp"}
    for call in rec["calls"].values():
        args = [_make(a) for a in call["args"]]
        kwargs = {k: _make(v) for k, v in call["kwargs"].items()}
        with pytest.raises(RuntimeError, match="no CPU path|need GPU tensors"):
            getattr(_C.ops, call["op"])(*args, **kwargs)
