"""reference: nunchaku/models/transformers/transformer_sana.py."""
from nunchaku_amd.models.transformer_sana import (  # noqa: F401
    NunchakuSanaTransformer2DModel,
    NunchakuSanaTransformerBlocks,
    inject_quantized_module,
    load_quantized_module,
)
