"""reference: nunchaku/models/pulid (the identity cross-attention modules and the forward; the face stack is not part of this library)."""
