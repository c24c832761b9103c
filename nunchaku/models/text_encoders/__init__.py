"""reference: nunchaku/models/text_encoders/__init__.py (transformers is imported on first access of NunchakuT5EncoderModel)."""
from nunchaku_amd.models.text_encoders import W4Linear  # noqa: F401


def __getattr__(name):
    if name == "NunchakuT5EncoderModel":
        from nunchaku_amd.models.text_encoders.t5_encoder import NunchakuT5EncoderModel

        return NunchakuT5EncoderModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
