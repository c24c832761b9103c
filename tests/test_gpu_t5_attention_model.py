"""The 4-bit T5 encoder on ``fused_t5_attention`` and on transformers' eager attention, both against the encoder with its attention in float64."""

import pytest
import torch

from tests.test_awq_gemm_host import write_tiny_t5_checkpoint

pytestmark = pytest.mark.gpu


def _f64_attention(module, query, key, value, attention_mask, **kw):
    from transformers.models.t5.modeling_t5 import eager_attention_forward

    out, _ = eager_attention_forward(module, query.double(), key.double(), value.double(), None if attention_mask is None else attention_mask.double(),
                                     **{**kw, "position_bias": kw["position_bias"].double()})
    return out.to(query.dtype), None


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "padding-mask"])
def test_the_fused_encoder_is_as_close_to_float64_attention_as_the_eager_one(tmp_path, monkeypatch, masked):
    from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS, eager_mask
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    import nunchaku_amd.ops.attention as A
    from nunchaku import NunchakuT5EncoderModel

    path, _, _ = write_tiny_t5_checkpoint(tmp_path / "t5.safetensors")
    fused, eager, exact = (NunchakuT5EncoderModel.from_pretrained(str(path), device="cuda", fused_attention=f) for f in (True, False, False))
    ALL_ATTENTION_FUNCTIONS.register("test_t5_float64", _f64_attention)
    ALL_MASK_ATTENTION_FUNCTIONS.register("test_t5_float64", eager_mask)
    eager.config._attn_implementation, exact.config._attn_implementation = "eager", "test_t5_float64"
    try:
        calls, op = [], A.attention_d64_bias
        monkeypatch.setattr(A, "attention_d64_bias", lambda *a, **k: calls.append(a[5] if len(a) > 5 else k.get("key_bias")) or op(*a, **k))
        ids = torch.randint(0, 128, (2, 77), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        mask = (torch.arange(77, device="cuda")[None, :] < torch.tensor([[77], [50]], device="cuda")).long() if masked else None
        with torch.no_grad():
            got = fused(input_ids=ids, attention_mask=mask).last_hidden_state.double()
            assert len(calls) == 2 and all((kb is not None) == masked for kb in calls)  # both layers took the kernel, the mask as key_bias
            ref = exact(input_ids=ids, attention_mask=mask).last_hidden_state.double()
            base = eager(input_ids=ids, attention_mask=mask).last_hidden_state.double()
        err, err_eager = (got - ref).abs().max().item(), (base - ref).abs().max().item()
        print(f"masked={masked}: fused encoder error {err:.3g}, eager encoder error {err_eager:.3g} (max |ref| {ref.abs().max().item():.3g})")
        assert torch.isfinite(got).all() and err <= 1.5 * err_eager
    finally:
        ALL_ATTENTION_FUNCTIONS._global_mapping.pop("test_t5_float64", None)
        ALL_MASK_ATTENTION_FUNCTIONS._global_mapping.pop("test_t5_float64", None)
