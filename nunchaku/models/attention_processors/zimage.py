"""reference: nunchaku/models/attention_processors/zimage.py."""
from nunchaku_amd.models.zimage import NunchakuZSingleStreamAttnProcessor  # noqa: F401
