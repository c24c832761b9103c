"""reference: nunchaku/models/pulid/pulid_forward.py."""
from nunchaku_amd.models.pulid import pulid_forward  # noqa: F401
