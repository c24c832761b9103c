"""reference: nunchaku/models/transformers/transformer_zimage.py."""
from nunchaku_amd.models.zimage import (  # noqa: F401
    NunchakuZImageAttention,
    NunchakuZImageFeedForward,
    NunchakuZImageSwiGLU,
    NunchakuZImageTransformer2DModel,
    NunchakuZImageTransformerBlock,
    ZImageBlockStack,
    ZImageSwiGLUFeedForward,
    patch_scale_key,
)
