"""reference: nunchaku/models/pulid/encoders_transformer.py (``PerceiverAttentionCA``; the ``IDFormer`` encoder is not part of this library)."""
from nunchaku_amd.models.pulid import PerceiverAttentionCA  # noqa: F401
