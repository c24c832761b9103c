"""reference: nunchaku/lora/flux (``compose_lora``; the converter's role is ``to_engine_lora`` here)."""
from nunchaku_amd.lora.flux import compose_lora, is_nunchaku_format, load_state_dict, to_engine_lora  # noqa: F401
