"""The 4-bit T5 text encoder (reference: nunchaku/models/text_encoders/).  ``W4Linear`` and the tinychat packer need only
torch; ``NunchakuT5EncoderModel`` needs transformers, which is imported on first access."""
from .linear import W4Linear  # noqa: F401
from .tinychat_utils import ceil_num_groups, convert_to_tinychat_w4x16y16_linear_weight  # noqa: F401

__all__ = ["NunchakuT5EncoderModel", "W4Linear", "ceil_num_groups", "convert_to_tinychat_w4x16y16_linear_weight"]


def __getattr__(name):
    if name == "NunchakuT5EncoderModel":
        from .t5_encoder import NunchakuT5EncoderModel

        return NunchakuT5EncoderModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
