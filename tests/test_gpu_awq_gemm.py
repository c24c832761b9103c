"""AWQ W4A16 GEMM (group 128, ops.gemm_awq) and the 4-bit T5 encoder on the GPU: the dequantisation bit for bit, parity with a
float64 restatement at the T5-XXL shapes (with and without the K-split), reproducibility, the fused bias, the reference's
positional surface, and the encoder end to end against a dense transformers T5 holding the dequantised weights."""
import numpy as np
import pytest
import torch

from nunchaku_amd.models.text_encoders import W4Linear
from nunchaku_amd.models.text_encoders.tinychat_utils import _pack_codes
from tests.helpers import assert_close_16
from tests.test_awq_gemm_host import dequantise, write_tiny_t5_checkpoint

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def make_layer(N, K, dtype, seed=0, G_pad=None):
    """random codes, scales in [0.004, 0.03), zeros = -z * scale with z in [0, 16): the checkpoint buffers on cuda"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    G = K // 128
    G_pad = G_pad or G
    codes = torch.randint(0, 16, (N, K), device="cuda", generator=g)
    s = (torch.rand(G, N, device="cuda", generator=g) * 0.026 + 0.004).to(dtype)
    z = -(torch.randint(0, 16, (G, N), device="cuda", generator=g).float() * s.float()).to(dtype)
    scales = torch.zeros(G_pad, N, dtype=dtype, device="cuda")
    zeros = torch.zeros(G_pad, N, dtype=dtype, device="cuda")
    scales[:G], zeros[:G] = s, z
    return _pack_codes(codes), scales, zeros


def gemm(x, qw, sc, zr, bias=None):
    from nunchaku_amd._C import ops

    return ops.gemm_awq(x, qw, sc, zr, bias=bias)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(192, 640), (256, 1024)])
def test_identity_rows_give_the_dequantised_weights_bit_exact(dtype, N, K):
    """x = I (M = K): out[m, n] = w16[n, m] with exactly one nonzero product, so any layout, group-index, padding-row or rounding
    error shows.  K = 640: 5 groups with the scale rows padded to 8; N = 192: a half output tile"""
    qw, sc, zr = make_layer(N, K, DT[dtype], seed=K, G_pad=8)
    x = torch.eye(K, dtype=DT[dtype], device="cuda")
    out = gemm(x, qw, sc, zr)
    torch.cuda.synchronize()
    w16 = dequantise(qw, sc, zr, K).cuda()
    assert torch.equal(out, w16.t().contiguous())


SHAPES = [(1, 64, 128), (7, 256, 640), (8, 4096, 4096), (300, 1536, 1024), (512, 4096, 4096), (512, 10240, 4096), (512, 4096, 10240),
          (1024, 4096, 4096)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_parity_with_float64_restatement(dtype, M, N, K):
    """round16(sum_k w16 x in float64) against the kernel's fp32 sums: 1 ulp, a small fraction of elements allowed past it
    (fp32 summation order; as the GEMV test).  The T5-XXL projections at 1 and 2 prompts, with ((512, 4096, K), (8, ...)) and
    without ((1024, ...), (512, 10240, 4096)) the K-split"""
    qw, sc, zr = make_layer(N, K, DT[dtype], seed=M + N + K)
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, K, device="cuda", generator=g).to(DT[dtype])
    out = gemm(x, qw, sc, zr)
    w16 = dequantise(qw, sc, zr, K).cuda()
    ref = (x.double() @ w16.double().t()).to(DT[dtype])
    assert out.shape == (M, N) and out.dtype == DT[dtype]
    assert_close_16(out.float().cpu().numpy(), ref.float().cpu().numpy(), dtype, f"gemm_awq {M}x{N}x{K}", max_bad_frac=2e-3)


@pytest.mark.parametrize("M,N,K", [(8, 4096, 4096), (512, 4096, 4096), (300, 1536, 1024)])
def test_reproducible_strided_and_3d(M, N, K):
    qw, sc, zr = make_layer(N, K, torch.bfloat16, seed=3)
    g = torch.Generator(device="cuda").manual_seed(1)
    xw = torch.randn(M, K + 64, device="cuda", generator=g).bfloat16()
    x = xw[:, :K]  # row stride K + 64
    a, b = gemm(x, qw, sc, zr), gemm(x, qw, sc, zr)
    c = gemm(x.contiguous(), qw, sc, zr)
    assert torch.equal(a, b) and torch.equal(a, c)
    if M % 4 == 0:
        d = gemm(x.contiguous().view(4, M // 4, K), qw, sc, zr)
        assert d.shape == (4, M // 4, N) and torch.equal(d.view(M, N), a)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("M", [8, 512, 1024])
def test_fused_bias_is_the_16_bit_add(dtype, M):
    N, K = 4096, 4096
    qw, sc, zr = make_layer(N, K, DT[dtype], seed=5)
    x = torch.randn(M, K, device="cuda").to(DT[dtype])
    bias = torch.randn(N, device="cuda").to(DT[dtype])
    assert torch.equal(gemm(x, qw, sc, zr, bias=bias), gemm(x, qw, sc, zr) + bias)


def test_reference_surface_positional_and_errors():
    from nunchaku._C import ops

    N, K = 256, 640
    qw, sc, zr = make_layer(N, K, torch.bfloat16, seed=9, G_pad=8)
    x = torch.randn(3, 5, K, device="cuda").bfloat16()
    y = ops.gemm_awq(x, qw, sc, zr)
    assert y.shape == (3, 5, N)
    # the same bytes as the GEMV's int32 [N/4, K/2] view
    assert torch.equal(ops.gemm_awq(x, qw.view(torch.int32), sc, zr), y)
    with pytest.raises(ValueError):
        ops.gemm_awq(x[..., :512], qw, sc, zr)  # K does not match the codes
    with pytest.raises(ValueError):
        ops.gemm_awq(x, qw, sc[:4], zr[:4])  # fewer than K/128 scale rows
    with pytest.raises(ValueError):
        ops.gemm_awq(x.half(), qw, sc, zr)  # dtype mismatch
    lin = W4Linear(K, N, group_size=64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError):
        lin(x)


def _compare_hidden(got, ref, what):
    """cosine >= 0.9999 per token and max |diff| <= 4 bf16 ulps of the token's max |ref|.  Both models round every linear output to bf16
    at the same points from the same w16; they differ only in fp32 summation order (1-ulp flips on a small fraction of outputs), which
    the layer norms, the softmax and the residual stream carry on at the size of those flips -- a layout or scale error is O(1)."""
    got, ref = got.float().flatten(0, -2), ref.float().flatten(0, -2)
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    rowmax = ref.abs().amax(dim=-1)
    ulp = torch.exp2(torch.floor(torch.log2(rowmax)) - 7)
    dmax = ((got - ref).abs().amax(dim=-1) / ulp)
    print(f"{what}: min cosine {cos.min().item():.7f}, max |diff| {dmax.max().item():.2f} bf16 ulps of the row max")
    assert cos.min().item() >= 0.9999, what
    assert dmax.max().item() <= 4.0, what


def test_tiny_t5_encoder_end_to_end(tmp_path):
    pytest.importorskip("transformers")
    from nunchaku import NunchakuT5EncoderModel

    path, dense, _ = write_tiny_t5_checkpoint(tmp_path / "t5.safetensors")
    model = NunchakuT5EncoderModel.from_pretrained(str(path), device="cuda")
    dense = dense.cuda()
    ids = torch.randint(0, 128, (2, 77), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    with torch.no_grad():
        got = model(input_ids=ids).last_hidden_state
        ref = dense(input_ids=ids).last_hidden_state
    _compare_hidden(got, ref, "tiny T5 (2 layers, gated-gelu, d_ff 640)")


def test_t5_xxl_sized_layer_at_512_tokens():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = transformers.T5Config(vocab_size=256, d_model=4096, d_kv=64, d_ff=10240, num_layers=1, num_heads=64, feed_forward_proj="gated-gelu",
                                dropout_rate=0.0, is_encoder_decoder=False, use_cache=False)
    with torch.device("cuda"):
        dense = transformers.T5EncoderModel(cfg).bfloat16().eval()
    with torch.no_grad():
        for p in dense.parameters():
            p.copy_(torch.randn_like(p.float()).mul(1.0 / 64).bfloat16())
        for name, mod in list(dense.named_modules()):
            for cname, child in list(mod.named_children()):
                if isinstance(child, torch.nn.Linear):
                    q = W4Linear.from_linear(child, group_size=128)
                    child.weight.copy_(dequantise(q.qweight, q.scales, q.scaled_zeros, child.in_features).cuda())
                    setattr(mod, cname, q)
                    q.weight = torch.empty(0, dtype=torch.bfloat16, device="meta")
                    q.dense = child  # keep the dequantised dense twin for the reference pass
    quant_ids = torch.randint(0, 256, (1, 512), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    with torch.no_grad():
        got = dense(input_ids=quant_ids).last_hidden_state
        for name, mod in list(dense.named_modules()):
            for cname, child in list(mod.named_children()):
                if isinstance(child, W4Linear):
                    setattr(mod, cname, child.dense)
        ref = dense(input_ids=quant_ids).last_hidden_state
    _compare_hidden(got, ref, "T5-XXL-sized layer (d_model 4096, d_ff 10240, 64 heads), 512 tokens")
