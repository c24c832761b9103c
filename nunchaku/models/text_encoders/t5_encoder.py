"""reference: nunchaku/models/text_encoders/t5_encoder.py (imports transformers)."""
from nunchaku_amd.models.text_encoders.t5_encoder import NunchakuT5EncoderModel  # noqa: F401
