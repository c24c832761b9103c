"""Stable Diffusion XL's quantised transformer block on the GPU, at its two widths (640 with 10 heads, 1280 with 20), batch 2 (classifier-free
guidance), a 2048-wide text condition of 77 tokens, both dtypes, synthetic weights (``synthetic_codes_``): every module against its
composition from the public pieces, bit for bit, and the attention inside the block against the accuracy gate of
tests/test_gpu_attention_d64.py with ``F.scaled_dot_product_attention`` in fp32 as the reference."""

import json
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DTYPES = ["bf16", "fp16"]
WIDTHS = [(640, 10), (1280, 20)]
B, CROSS, TXT = 2, 2048, 77


@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


@torch.no_grad()
def _init_synthetic_(block, seed):
    """random weights in the checkpoint layout, as models/blocks.py::init_synthetic_ draws them for a W4A4 layer; LayerNorms near (1, 0)"""
    from nunchaku_amd.models.linear import SVDQW4A4Linear, synthetic_codes_

    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda shape, scale: torch.randn(tuple(shape), generator=g, device="cuda") * scale
    for m in block.modules():
        if isinstance(m, SVDQW4A4Linear):
            K = m.in_features
            synthetic_codes_(m.qweight, m.wscales, K, g)
            if m.bias is not None:
                m.bias.copy_(rnd(m.bias.shape, 0.02))
            m.smooth_factor.copy_(torch.rand((K,), generator=g, device="cuda") + 0.5)
            m.smooth_factor_orig.copy_(m.smooth_factor)
            m.proj_down.copy_(rnd(m.proj_down.shape, 0.5 / math.sqrt(K)))
            m.proj_up.copy_(rnd(m.proj_up.shape, 0.5 / math.sqrt(m.rank)))
        elif isinstance(m, torch.nn.Linear):
            m.weight.copy_(rnd(m.weight.shape, 1.0 / math.sqrt(m.in_features)))
        elif isinstance(m, torch.nn.LayerNorm):
            m.weight.copy_(1.0 + rnd(m.weight.shape, 0.1))
            m.bias.copy_(rnd(m.bias.shape, 0.1))
    return block


_BLOCKS = {}


def _block(dim, heads, dtype):
    """one block per width and dtype, built once and left unchanged"""
    from nunchaku_amd.models.sdxl import NunchakuSDXLTransformerBlock

    if (dim, dtype) not in _BLOCKS:
        blk = NunchakuSDXLTransformerBlock(dim, heads, CROSS, rank=32, torch_dtype=TD[dtype], device="cuda")
        _BLOCKS[dim, dtype] = _init_synthetic_(blk, seed=dim + (dtype == "fp16"))
    return _BLOCKS[dim, dtype]


def _acts(dim, T, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + dim + T)
    x = torch.randn(B, T, dim, device="cuda", generator=g).to(TD[dtype])
    enc = torch.randn(B, TXT, CROSS, device="cuda", generator=g).to(TD[dtype])
    return x, enc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads", WIDTHS)
def test_attention_modules_equal_their_composition(dim, heads, dtype, strict_mode):
    from nunchaku_amd.ops import attention_d64

    blk = _block(dim, heads, dtype)
    x, enc = _acts(dim, 96, dtype)
    # self-attention: to_qkv -> attention_d64 on the thirds in place -> to_out[0] -> the 16-bit divide
    a = blk.attn1
    y = a(x)
    assert y.shape == x.shape and y.dtype == TD[dtype] and torch.isfinite(y).all() and y.float().abs().max() > 0.01
    assert torch.equal(a(x), y)                                                                        # a second call
    qkv = a.to_qkv(x)
    o = attention_d64(qkv[..., :dim], qkv[..., dim:2 * dim], qkv[..., 2 * dim:], heads)
    assert torch.equal(y, a.to_out[0](o) / a.rescale_output_factor)
    a.rescale_output_factor = 3.0
    try:
        assert torch.equal(a(x), a.to_out[0](o) / 3.0)
    finally:
        a.rescale_output_factor = 1.0
    # cross-attention: to_q quantised, to_k / to_v unquantised on the text
    c = blk.attn2
    yc = c(x, encoder_hidden_states=enc)
    assert yc.shape == x.shape and torch.isfinite(yc).all() and yc.float().abs().max() > 0.01
    oc = attention_d64(c.to_q(x), c.to_k(enc), c.to_v(enc), heads)
    assert torch.equal(yc, c.to_out[0](oc) / c.rescale_output_factor)
    assert not torch.equal(yc[0], c(x, encoder_hidden_states=enc.flip(0))[0])                           # (the text is looked at)
    with pytest.raises(NotImplementedError, match="attention_mask is not supported"):
        a(x, attention_mask=torch.zeros(B, 96, device="cuda"))


def _gate(out, q, k, v, heads, dtype, what):
    """tests/test_gpu_attention_d64.py's gate with F.scaled_dot_product_attention in fp32 as the reference"""
    split = lambda t, dt: t.to(dt).reshape(t.shape[0], t.shape[1], heads, 64).transpose(1, 2)
    merge = lambda t: t.transpose(1, 2).reshape(out.shape)
    ref = merge(F.scaled_dot_product_attention(split(q, torch.float32), split(k, torch.float32), split(v, torch.float32)))
    low = merge(F.scaled_dot_product_attention(split(q, q.dtype), split(k, q.dtype), split(v, q.dtype)))
    err, err_sdpa = (out.float() - ref).abs().max().item(), (low.float() - ref).abs().max().item()
    tol = 3 * ULP[dtype] * ref.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), torch 16-bit SDPA {err_sdpa:.3g}")
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g}"
    assert err <= 1.5 * err_sdpa + 1e-6, f"{what}: error {err:.3g} vs torch 16-bit SDPA {err_sdpa:.3g}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads", WIDTHS)
def test_block_equals_its_composition_and_its_attention_passes_the_gate(dim, heads, dtype, strict_mode):
    from nunchaku_amd.ops import attention_d64

    blk = _block(dim, heads, dtype)
    x, enc = _acts(dim, 64, dtype, seed=1)                # 64 tokens: half a query tile
    y = blk(x, encoder_hidden_states=enc)
    assert y.shape == x.shape and y.dtype == TD[dtype] and torch.isfinite(y).all()
    assert torch.equal(blk(x, encoder_hidden_states=enc), y)
    # the three sub-modules, nn.LayerNorm and 16-bit adds
    n1 = F.layer_norm(x, (dim,), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    h = blk.attn1(n1) + x
    n2 = F.layer_norm(h, (dim,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
    h = blk.attn2(n2, encoder_hidden_states=enc) + h
    n3 = F.layer_norm(h, (dim,), blk.norm3.weight, blk.norm3.bias, blk.norm3.eps)
    assert torch.equal(y, blk.ff(n3) + h)
    # the feed-forward: GEGLU as diffusers computes it, in the 16-bit dtype
    hg, g = blk.ff.net[0].proj(n3).chunk(2, dim=-1)
    assert torch.equal(blk.ff(n3), blk.ff.net[2](hg * F.gelu(g)))
    # the attention sub-steps on the block's own projections
    qkv = blk.attn1.to_qkv(n1)
    q, k, v = qkv[..., :dim], qkv[..., dim:2 * dim], qkv[..., 2 * dim:]
    _gate(attention_d64(q, k, v, heads), q, k, v, heads, dtype, f"self-attention of the block ({dim}, {dtype})")
    q, k, v = blk.attn2.to_q(n2), blk.attn2.to_k(enc), blk.attn2.to_v(enc)
    _gate(attention_d64(q, k, v, heads), q, k, v, heads, dtype, f"cross-attention of the block ({dim}, {dtype})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads", WIDTHS)
def test_a_4d_input_equals_the_3d_path(dim, heads, dtype, strict_mode):
    blk = _block(dim, heads, dtype)
    g = torch.Generator(device="cuda").manual_seed(dim)
    x4 = torch.randn(B, dim, 8, 8, device="cuda", generator=g).to(TD[dtype])
    _, enc = _acts(dim, 64, dtype, seed=2)
    x3 = x4.view(B, dim, 64).transpose(1, 2).contiguous()
    for attn, kw in ((blk.attn1, {}), (blk.attn2, dict(encoder_hidden_states=enc))):
        y4 = attn(x4, **kw)
        assert y4.shape == x4.shape
        assert torch.equal(y4, attn(x3, **kw).transpose(-1, -2).reshape(B, dim, 8, 8))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_checkpoint_round_trip_reproduces_the_block(tmp_path, dtype, strict_mode):
    from safetensors.torch import save_file

    from nunchaku_amd.models import sdxl
    from tests.test_sdxl import _legacy

    dim, heads = 640, 10
    blk = _block(dim, heads, dtype)
    x, enc = _acts(dim, 64, dtype, seed=3)
    want = blk(x, encoder_hidden_states=enc)
    pre = "down_blocks.1.attentions.0.transformer_blocks.1"
    sd = {f"{pre}.{_legacy(k)}": v.detach().cpu().contiguous() for k, v in blk.state_dict().items()}   # the checkpoint's names and layout
    assert f"{pre}.attn1.to_qkv.lora_down" in sd and f"{pre}.ff.net.2.smooth_orig" in sd
    sd["conv_in.bias"] = torch.zeros(320, dtype=TD[dtype])
    path = str(tmp_path / "sdxl_tiny.safetensors")
    save_file(sd, path, metadata={"config": json.dumps(dict(cross_attention_dim=CROSS)), "quantization_config": json.dumps({"rank": 32})})
    if sdxl.HAVE_DIFFUSERS:  # the class then builds diffusers' own skeleton (tests/test_sdxl.py runs that build): the converter and a block alone
        fresh = sdxl.NunchakuSDXLTransformerBlock(dim, heads, CROSS, torch_dtype=TD[dtype], device="cuda")
        conv = sdxl.convert_sdxl_state_dict(sdxl.NunchakuSDXLUNet2DConditionModel._read_safetensors(path)[0])
        fresh.load_state_dict({k[len(pre) + 1:]: v for k, v in conv.items() if k.startswith(pre)}, strict=True)
    else:
        unet = sdxl.NunchakuSDXLUNet2DConditionModel.from_pretrained(path, device="cuda", torch_dtype=TD[dtype])
        assert unet.transformer_block_names == [pre] and set(unet.unquantized_state_dict) == {"conv_in.bias"}
        assert unet.device.type == "cuda" and unet.dtype == TD[dtype]
        with pytest.raises(RuntimeError, match="diffusers"):
            unet(x)
        fresh = unet.transformer_block(pre)
    assert fresh is not blk and fresh.attn1.heads == heads
    assert torch.equal(fresh(x, encoder_hidden_states=enc), want)
