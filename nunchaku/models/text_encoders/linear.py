"""reference: nunchaku/models/text_encoders/linear.py."""
from nunchaku_amd.models.text_encoders.linear import W4Linear  # noqa: F401
