"""reference: nunchaku/models/ip_adapter/utils.py (the adapter is state on the engine here: ``IPAdapter``, not a block wrapper)."""
from nunchaku_amd.models.ip_adapter import IPAdapter, resize_numpy_image_long, undo_all_mods_on_transformer  # noqa: F401
