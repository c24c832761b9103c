"""reference: nunchaku/models/text_encoders/tinychat_utils.py."""
from nunchaku_amd.models.text_encoders.tinychat_utils import ceil_num_groups, convert_to_tinychat_w4x16y16_linear_weight  # noqa: F401
