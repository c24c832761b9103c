"""LoRA loading for the engine models: diffusers / PEFT state dicts -> per-layer factors (``nunchaku_amd.lora.flux``)."""
