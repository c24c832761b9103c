"""The 4-bit T5 encoder with ``fused_layers`` on and off, both against its dense twin in float64."""
import pytest
import torch

from tests.test_awq_gemm_host import write_tiny_t5_checkpoint

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "padding-mask"])
def test_the_fused_encoder_is_as_close_to_the_float64_twin_as_the_parent_path(tmp_path, monkeypatch, masked):
    import nunchaku_amd.ops.gemm as G
    from nunchaku import NunchakuT5EncoderModel

    path, dense, _ = write_tiny_t5_checkpoint(tmp_path / "t5.safetensors")
    plain, off, fused = (NunchakuT5EncoderModel.from_pretrained(str(path), device="cuda", **kw) for kw in ({}, {"fused_layers": False}, {"fused_layers": True}))
    dense = dense.cuda().double()
    assert list(fused.state_dict()) == list(plain.state_dict()) == list(fused.set_fused_layers(False).state_dict())
    fused.set_fused_layers(True)
    calls, op = [], G.gemm_awq_multi
    monkeypatch.setattr(G, "gemm_awq_multi", lambda x, w, mode="concat", out=None: calls.append(mode) or op(x, w, mode, out))
    ids = torch.randint(0, 128, (2, 77), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    mask = (torch.arange(77, device="cuda")[None, :] < torch.tensor([[77], [50]], device="cuda")).long() if masked else None
    with torch.no_grad():
        got = fused(input_ids=ids, attention_mask=mask).last_hidden_state
        assert sorted(calls) == ["concat"] * 2 + ["gated_gelu_new"] * 2  # each of the two layers: one CONCAT and one GATED launch
        base = off(input_ids=ids, attention_mask=mask).last_hidden_state
        assert len(calls) == 4 and torch.equal(base, plain(input_ids=ids, attention_mask=mask).last_hidden_state)
        ref = dense(input_ids=ids, attention_mask=mask).last_hidden_state
    err, err_parent = ((t.double() - ref).abs().max().item() for t in (got, base))
    print(f"masked={masked}: fused encoder error {err:.3g}, parent path error {err_parent:.3g} (max |ref| {ref.abs().max().item():.3g})")
    assert torch.isfinite(got).all() and err <= 1.5 * err_parent
