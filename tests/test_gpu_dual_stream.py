"""The FLUX joint block and the Qwen-Image block are ONE computation on the fused path (models/blocks.py): the same weights, rotary
tables, modulation input and LayerNorm statistics through ``FluxJointBlockAMD.forward(..., stats=...)`` and through
``NunchakuQwenImageTransformerBlock.forward_fused`` give the same bits -- both output streams and both statistics tensors."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
DIM, HEADS, RANK = 256, 2, 32
# FLUX sub-module prefix -> Qwen-Image sub-module prefix
NAME_MAP = (("norm1.linear.", "img_mod.1."), ("norm1_context.linear.", "txt_mod.1."), ("ff.", "img_mlp."), ("ff_context.", "txt_mlp."),
            ("attn.", "attn."))


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _blocks(dt):
    """A FLUX joint block with synthetic weights (checkpoint layout) and a Qwen-Image block holding copies of them."""
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformerBlock

    model = FluxTransformerAMD(num_layers=1, num_single_layers=0, dim=DIM, heads=HEADS, in_channels=64, joint_attention_dim=128,
                               pooled_projection_dim=64, rank=RANK, torch_dtype=dt, device="cuda").init_synthetic_(seed=3, repack=False)
    fb = model.transformer_blocks[0]
    g = torch.Generator(device="cuda").manual_seed(4)
    for norm in (fb.attn.norm_q, fb.attn.norm_k, fb.attn.norm_added_q, fb.attn.norm_added_k):  # four different weights: a mix-up shows
        norm.weight.copy_((1 + 0.1 * torch.randn(128, device="cuda", generator=g)).to(dt))
    qb = NunchakuQwenImageTransformerBlock(DIM, HEADS, DIM // HEADS, rank=RANK, scale_shift=0.0, torch_dtype=dt, device="cuda")
    sd = {}
    for k, v in fb.state_dict().items():
        src, dst = next(p for p in NAME_MAP if k.startswith(p[0]))
        sd[dst + k[len(src):]] = v.clone()
    qb.load_state_dict(sd)  # strict: every parameter of either block has its counterpart in the other
    return fb.eval(), qb.eval()


@pytest.mark.parametrize("name,t_txt,grid", [("bf16", 256, (16, 16)), ("fp16", 256, (16, 16)), ("bf16", 77, (15, 20))],
                         ids=["bf16-256+256", "fp16-256+256", "bf16-padded-77+300"])
def test_flux_and_qwen_fused_blocks_are_bit_equal(name, t_txt, grid):
    """256 + 256 rows: one 256-row tile per stream, the smallest shape the grouped launches take.  77 + 300 tokens: padded to 256 + 512
    rows (zero rows, as the engines pad) with the attention's key ranges.  fp16: Qwen clips both streams at the end of the block, FLUX the
    text stream only -- the image stream stays far below 65504 here (asserted), so the clip cannot make them differ."""
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import pack_qwen_rotary, qwen_rope_freqs
    from nunchaku_amd.ops.attention import kv_valid_ranges
    from nunchaku_amd.ops.elementwise import residual_gate_stats

    dt = DTYPES[name]
    t_img = grid[0] * grid[1]
    p_txt, p_img = -(-t_txt // 256) * 256, -(-t_img // 256) * 256
    with torch.no_grad(), mode.deterministic_mode():
        fb, qb = _blocks(dt)
        g = torch.Generator(device="cuda").manual_seed(7)
        hidden = torch.zeros(1, p_img, DIM, dtype=dt, device="cuda")
        enc = torch.zeros(1, p_txt, DIM, dtype=dt, device="cuda")
        hidden[:, :t_img] = torch.randn(1, t_img, DIM, device="cuda", generator=g).to(dt)
        enc[:, :t_txt] = torch.randn(1, t_txt, DIM, device="cuda", generator=g).to(dt)
        temb_act = torch.nn.functional.silu(torch.randn(1, DIM, device="cuda", generator=g).to(dt))
        rot = pack_qwen_rotary(*qwen_rope_freqs((1, *grid), t_txt, device="cuda"))
        kv_valid = kv_valid_ranges(t_txt, t_img)
        assert (kv_valid is None) == (t_txt == p_txt and t_img == p_img)
        stats = lambda: ((residual_gate_stats(hidden)[1], None), (residual_gate_stats(enc)[1], None))  # (image, text), each with its pool

        # both blocks update the streams in place: each gets its own copies
        f_enc, f_hid, ((f_hs, _), (f_es, _)) = fb(hidden.clone(), enc.clone(), temb_act, (rot["img"], rot["txt"], rot["all"]), stats=stats(),
                                                  kv_valid=kv_valid)
        q_enc, q_hid, ((q_hs, _), (q_es, _)) = qb.forward_fused(hidden.clone(), enc.clone(), temb_act, rot, stats(), kv_valid=kv_valid)
        torch.cuda.synchronize()

    for label, t in (("image", f_hid), ("text", f_enc), ("image statistics", f_hs), ("text statistics", f_es)):
        assert torch.isfinite(t.float()).all(), label
    assert not torch.equal(f_hid, hidden) and not torch.equal(f_enc, enc)  # the block ran
    peak = f_hid.float().abs().max().item()
    print(f"{name} {t_txt}+{t_img}: image stream peak {peak:.3f}")
    if dt == torch.float16:
        assert peak < 65504
    for label, a, b in (("image stream", f_hid, q_hid), ("text stream", f_enc, q_enc), ("image statistics", f_hs, q_hs),
                        ("text statistics", f_es, q_es)):
        assert a.shape == b.shape and a.dtype == b.dtype, label
        n = (a != b).sum().item()
        print(f"{name} {t_txt}+{t_img}: {label}: {n} of {a.numel()} elements differ")
        assert torch.equal(a, b), f"{label}: FLUX and Qwen-Image differ in {n} elements"
