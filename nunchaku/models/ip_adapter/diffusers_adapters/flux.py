"""reference: nunchaku/models/ip_adapter/diffusers_adapters/flux.py."""
from nunchaku_amd.models.ip_adapter import apply_IPA_on_pipe, apply_IPA_on_transformer, undo_all_mods_on_transformer  # noqa: F401
