"""reference: nunchaku/models/unets/unet_sdxl.py."""
from nunchaku_amd.models.sdxl import (  # noqa: F401
    NunchakuSDXLAttention,
    NunchakuSDXLFeedForward,
    NunchakuSDXLGEGLU,
    NunchakuSDXLTransformerBlock,
    NunchakuSDXLUNet2DConditionModel,
    convert_sdxl_state_dict,
)
