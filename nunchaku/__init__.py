"""``nunchaku`` import surface on MI355X: the reference's package layout re-exported from ``nunchaku_amd``.

``from nunchaku import NunchakuFluxTransformer2DModelV2`` / ``from nunchaku.models.linear import SVDQW4A4Linear`` /
``from nunchaku._C import ops`` / ``from nunchaku.ops.fused import fused_gelu_mlp`` resolve to the MI355X implementation
(reference: nunchaku/__init__.py:1-17, nunchaku/csrc/pybind.cpp:108-123).  ``nunchaku._C.ops`` takes the reference's
positional signatures, reference-sized opaque buffers and checkpoint-layout parameters (nunchaku_amd/_C.py), so the
reference's own ``ops/*.py`` / ``models/linear.py`` callers run against it unchanged (tests/test_nunchaku_shim.py).
``from nunchaku import NunchakuT5EncoderModel`` is the 4-bit T5 text encoder of the FLUX pipelines (AWQ W4A16 group-128
linears on ``ops.gemm_awq``); transformers is imported on first access of that name, so ``import nunchaku`` works without it.
``from nunchaku import NunchakuSanaTransformer2DModel`` is SANA (``nunchaku_amd/models/transformer_sana.py``).
``from nunchaku.models.unets.unet_sdxl import NunchakuSDXLUNet2DConditionModel`` is Stable Diffusion XL (``nunchaku_amd/models/sdxl.py``).
``from nunchaku import NunchakuZImageTransformer2DModel`` is Z-Image (``nunchaku_amd/models/zimage.py``).
"""
from .models import (  # noqa: F401
    NunchakuFluxTransformer2dModel,
    NunchakuFluxTransformer2DModelV2,
    NunchakuQwenImageTransformer2DModel,
    NunchakuSanaTransformer2DModel,
    NunchakuZImageTransformer2DModel,
)

__all__ = ["NunchakuFluxTransformer2dModel", "NunchakuFluxTransformer2DModelV2", "NunchakuQwenImageTransformer2DModel", "NunchakuSanaTransformer2DModel", "NunchakuZImageTransformer2DModel"]  # (+ NunchakuT5EncoderModel, lazily)


def __getattr__(name):
    if name == "NunchakuT5EncoderModel":
        from .models.text_encoders.t5_encoder import NunchakuT5EncoderModel

        return NunchakuT5EncoderModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
