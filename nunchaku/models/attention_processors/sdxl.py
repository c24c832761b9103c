"""reference: nunchaku/models/attention_processors/sdxl.py."""
from nunchaku_amd.models.sdxl import NunchakuSDXLFA2Processor  # noqa: F401
