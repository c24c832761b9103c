"""reference: nunchaku/models/ip_adapter."""
