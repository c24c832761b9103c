"""reference: nunchaku/models/unets/__init__.py (the shifted ResNet convolutions it also lists are unused there and are not part of this
package)."""
from .unet_sdxl import (  # noqa: F401
    NunchakuSDXLAttention,
    NunchakuSDXLFeedForward,
    NunchakuSDXLTransformerBlock,
    NunchakuSDXLUNet2DConditionModel,
)

__all__ = ["NunchakuSDXLAttention", "NunchakuSDXLTransformerBlock", "NunchakuSDXLUNet2DConditionModel", "NunchakuSDXLFeedForward"]
