"""reference: nunchaku/lora (the diffusers / PEFT -> engine converter for FLUX)."""
