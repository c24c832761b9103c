"""The T5 encoder's fused attention without a GPU: the Toeplitz vector behind ``compute_bias`` and the conditions that select transformers' eager function."""

import pytest
import torch

pytest.importorskip("transformers")


def _attention(heads=3, d_kv=64, decoder=False):
    from transformers.models.t5.modeling_t5 import T5Attention, T5Config

    torch.manual_seed(0)
    cfg = T5Config(d_model=32, d_kv=d_kv, num_heads=heads, d_ff=64, num_layers=1, vocab_size=16, is_decoder=decoder)
    return T5Attention(cfg, has_relative_attention_bias=True, layer_idx=0).eval()


@pytest.mark.parametrize("T,N", [(5, 9), (9, 5), (1, 7), (300, 300)])
def test_the_toeplitz_vector_reproduces_compute_bias(T, N):
    from nunchaku_amd.models.text_encoders.t5_encoder import toeplitz_rel_bias

    with torch.no_grad():
        pb = _attention().compute_bias(T, N)  # [1, H, T, N]
    rel = toeplitz_rel_bias(pb)
    assert rel.shape == (3, T + N - 1) and rel.dtype == torch.float32 and rel.is_contiguous()
    idx = torch.arange(N)[None, :] - torch.arange(T)[:, None] + T - 1
    assert torch.equal(rel[:, idx], pb[0].float()) and toeplitz_rel_bias(pb) is rel  # entry for entry; built once per tensor


def test_every_fallback_condition_selects_eager(monkeypatch):
    from nunchaku_amd.models.text_encoders import t5_encoder as M
    from transformers.models.t5 import modeling_t5

    B, H, T = 2, 3, 6
    attn = _attention(H)
    rows = lambda d=64: torch.randn(B, T, H * d).bfloat16().view(B, T, H, d).transpose(1, 2)
    good = dict(module=attn, query=rows(), key=rows(), value=rows(), attention_mask=None, dropout=0.0,
                position_bias=attn.compute_bias(T, T).detach().bfloat16())
    eager, real = [], modeling_t5.eager_attention_forward
    monkeypatch.setattr(modeling_t5, "eager_attention_forward", lambda *a, **k: eager.append(1) or real(*a, **k))
    M.fused_t5_attention(**good)                                             # a CPU tensor: eager, whatever the predicate says
    assert len(eager) == 1
    ok = torch.zeros(B, 1, 1, T).bfloat16()
    with torch.no_grad():
        assert all(M._serves(**{**good, "attention_mask": m}) for m in (None, ok, ok.expand(B, 1, T, T)))  # the three masks the kernel takes
        attn.train()
        assert not M._serves(**{**good, "dropout": 0.1})                     # training mode with dropout
        attn.eval()
        for case in (dict(attention_mask=torch.zeros(B, 1, T, T).bfloat16()),    # a mask that may vary along queries
                     dict(attention_mask=torch.zeros(B, H, 1, T).bfloat16()),    # ... along heads
                     dict(module=_attention(H, decoder=True)),                   # a decoder
                     dict(query=rows(32), key=rows(32), value=rows(32)),         # d_kv != 64
                     dict(query=rows().contiguous()),                            # not a view of token-major rows
                     dict(position_bias=good["position_bias"].expand(B, H, T, T))):  # a position bias with a batch dimension
            assert not M._serves(**{**good, **case}), case.keys()
