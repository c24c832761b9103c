"""svdq_ip_attention on the GPU: the image-prompt cross-attention of IP-Adapter (a few queries against at most 256 keys, Q read in
place from a packed QKV buffer, K / V as an nn.Linear wrote them) against the fp32 reference of tests/ipa_ref.py.  The accuracy gate is
the one of tests/test_gpu_attention.py: |err| <= 3 * 2^-8 (bf16) / 3 * 2^-11 (fp16) relative to max|ref|, and no worse than 1.5 x the
error of torch's own 16-bit SDPA on the same inputs."""

import math

import pytest
import torch

from tests.ipa_ref import ip_attention_ref

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
CASES = [(16, 1, 1), (48, 3, 4), (256, 2, 20), (300, 3, 128), (256, 1, 200), (128, 2, 256)]


def _inputs(T, H, N, dtype, seed=0):
    """packed qkv [T, 3*H*128] (half the query rows x 4: peaky rows) and the adapter's k / v [N, H*128]"""
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + N)
    qkv = torch.randn(T, 3 * H * 128, device="cuda", generator=g).to(TD[dtype])
    qkv[: T // 2, : H * 128] *= 4.0
    k = torch.randn(N, H * 128, device="cuda", generator=g).to(TD[dtype])
    v = torch.randn(N, H * 128, device="cuda", generator=g).to(TD[dtype])
    return qkv, k, v


def _prescaled(qkv, H):
    """tests/test_gpu_attention.py ``_as_produced_for``: the Q a producer multiplied by scale * log2(e) before rounding; the reference
    over the SAME 16-bit values then has the softmax scale ln 2"""
    from nunchaku_amd.ops.attention import q_prescale

    pre = qkv.clone()
    pre[:, : H * 128] = (qkv[:, : H * 128].float() * q_prescale(128)).to(qkv.dtype)
    return pre, math.log(2.0)


def _sdpa16(q, k, v, H, scale):
    shp = lambda t: t.reshape(1, -1, H, 128).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(shp(q.contiguous()), shp(k), shp(v), scale=scale)
    return o.transpose(1, 2).reshape(q.shape[0], H * 128)


def _gate(out, q, k, v, H, scale, dtype, what=""):
    ref = ip_attention_ref(q, k, v, H, scale)
    err = (out.float() - ref).abs().max().item()
    err_sdpa = (_sdpa16(q, k, v, H, scale).float() - ref).abs().max().item()
    tol = 3 * ULP[dtype] * ref.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), torch 16-bit SDPA {err_sdpa:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g}"
    assert err <= 1.5 * err_sdpa + 1e-6, f"{what}: error {err:.3g} vs torch 16-bit SDPA {err_sdpa:.3g}"


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("T,H,N", CASES)
def test_ip_attention_accuracy(T, H, N, dtype):
    from nunchaku_amd.ops.attention import ip_attention

    qkv, k, v = _inputs(T, H, N, dtype)
    out = ip_attention(qkv, k, v, H)
    assert out.shape == (T, H * 128) and out.dtype == TD[dtype]
    _gate(out, qkv[:, : H * 128], k, v, H, 1.0 / math.sqrt(128), dtype, f"({T},{H},{N}) {dtype} plain")
    assert torch.equal(ip_attention(qkv[:, : H * 128].contiguous(), k, v, H), out)  # a [T, H*128] Q is the same call
    pre, scale = _prescaled(qkv, H)
    out = ip_attention(pre, k, v, H, q_prescaled=True)
    _gate(out, pre[:, : H * 128], k, v, H, scale, dtype, f"({T},{H},{N}) {dtype} prescaled")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("T,H,N", [(48, 3, 4), (300, 3, 128), (256, 1, 200)])
def test_out_scale_multiplies_in_fp32_and_launches_are_bit_equal(T, H, N, dtype):
    from nunchaku_amd.ops.attention import ip_attention

    qkv, k, v = _inputs(T, H, N, dtype, seed=1)
    one = ip_attention(qkv, k, v, H, out_scale=1.0)
    assert torch.equal(one, ip_attention(qkv, k, v, H))
    scaled = ip_attention(qkv, k, v, H, out_scale=1.1)
    # torch's `1.1 * tensor`: the fp32 product with the fp32 scalar, rounded once -- the scalar itself is NOT rounded to 16 bits
    assert torch.equal(scaled, (torch.tensor(1.1, dtype=torch.float32, device="cuda") * one.float()).to(TD[dtype]))
    if dtype == "bf16":  # (torch's own fp16 kernel for `float * tensor` may round the exact product once -- a mixed-precision FMA -- and then
        assert torch.equal(scaled, 1.1 * one)  # differs from the two-step form above on ~2^-13 of the elements; bf16 has no such instruction)
    assert torch.equal(scaled, ip_attention(qkv, k, v, H, out_scale=1.1))  # no atomics: bit-equal from launch to launch
    assert not torch.equal(scaled, (one * torch.tensor(1.1, device="cuda").to(TD[dtype])))  # (a 16-bit scale would differ: the case is not vacuous)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("T,H,N", [(16, 1, 1), (256, 2, 20), (300, 3, 128), (256, 1, 200), (128, 2, 256)])
def test_nothing_outside_the_operands_is_read_or_written(T, H, N, dtype):
    """Every poison value sits in memory this test owns: the K and V thirds of the packed buffer and the buffer's rows beyond T are NaN,
    the rows of k / v beyond N are NaN / 6e4, the output is a column slice of the first T rows of a larger sentinel-filled buffer."""
    from nunchaku_amd.ops.attention import ip_attention

    qkv, k, v = _inputs(T, H, N, dtype, seed=2)
    hd = H * 128
    clean = ip_attention(qkv, k, v, H, out_scale=0.7)
    big_q = torch.full((T + 40, 3 * hd), float("nan"), device="cuda", dtype=TD[dtype])
    big_q[:T, :hd] = qkv[:, :hd]
    big_k = torch.full((N + 70, hd + 64), float("nan"), device="cuda", dtype=TD[dtype])
    big_v = torch.full((N + 70, hd + 64), 6e4, device="cuda", dtype=TD[dtype])
    big_k[:N, :hd], big_v[:N, :hd] = k, v
    sentinel = -77.0
    big_o = torch.full((T + 33, hd + 128), sentinel, device="cuda", dtype=TD[dtype])
    out = big_o[:T, 64:64 + hd]
    got = ip_attention(big_q[:T], big_k[:N, :hd], big_v[:N, :hd], H, out=out, out_scale=0.7)
    assert got is out and torch.isfinite(out).all() and torch.equal(out, clean)
    assert (big_o[T:] == sentinel).all() and (big_o[:T, :64] == sentinel).all() and (big_o[:T, 64 + hd:] == sentinel).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_softmax_edges(dtype):
    from nunchaku_amd.ops.attention import ip_attention

    T, H, N = 64, 2, 40
    g = torch.Generator(device="cuda").manual_seed(7)
    td, hd = TD[dtype], H * 128
    v = torch.randn(N, hd, device="cuda", generator=g).to(td)
    # one key ahead of all others by more than 100 in score: q = 12 * ones, k_star = ones -> 12 * 128 / sqrt(128) ~ 136, the others ~ 0
    k = (torch.randn(N, hd, device="cuda", generator=g) * 0.05).to(td)
    k[17] = 1.0
    q = torch.full((T, hd), 12.0, device="cuda", dtype=td)
    scores = torch.einsum("hd,nhd->hn", q.float().view(T, H, 128)[0], k.float().view(N, H, 128)) / math.sqrt(128)
    others = torch.cat([scores[:, :17], scores[:, 18:]], dim=1)
    assert (scores[:, 17] - others.max(dim=1).values).min().item() > 100
    out = ip_attention(q, k, v, H)
    _gate(out, q, k, v, H, 1.0 / math.sqrt(128), dtype, f"one dominant key {dtype}")
    assert torch.equal(out, v[17].expand(T, hd)), "a row dominated by one key returns that key's V row"
    # all keys equal: the mean of V
    k_same = k[3].expand(N, hd).contiguous()
    q = torch.randn(T, hd, device="cuda", generator=g).to(td)
    out = ip_attention(q, k_same, v, H)
    mean = v.float().mean(dim=0)
    assert (out.float() - mean).abs().max().item() <= 3 * ULP[dtype] * mean.abs().max().item()
    _gate(out, q, k_same, v, H, 1.0 / math.sqrt(128), dtype, f"all keys equal {dtype}")
    # scores near +-200 before the maximum is subtracted stay finite (fp16: exp(200) is far beyond the format)
    base = torch.randn(1, hd, device="cuda", generator=g)
    base = base / base.view(H, 128).norm(dim=1).repeat_interleave(128)[None]  # unit norm per head
    amp = math.sqrt(200.0 * math.sqrt(128))  # q . k = +-amp^2 -> scaled score +-200
    q = (base * amp).expand(T, hd).to(td).contiguous()
    q[T // 2:] *= -1
    k = (base * amp).expand(N, hd).to(td).contiguous()
    k[N // 2:] *= -1
    k = (k.float() + torch.randn(N, hd, device="cuda", generator=g) * 0.05).to(td)
    sc = (q.float().view(T, H, 128)[:, 0] @ k.float().view(N, H, 128)[:, 0].T) / math.sqrt(128)
    assert sc.max() > 150 and sc.min() < -150
    out = ip_attention(q, k, v, H)
    _gate(out, q, k, v, H, 1.0 / math.sqrt(128), dtype, f"scores near +-200 {dtype}")


def test_more_than_256_keys_and_other_head_dims_are_refused():
    from nunchaku_amd.ops.attention import ip_attention

    q = torch.zeros(16, 256, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="at most 256"):
        ip_attention(q, torch.zeros(257, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(257, 256, device="cuda", dtype=torch.bfloat16), 2)
    with pytest.raises(NotImplementedError, match="head_dim=64"):
        ip_attention(q, torch.zeros(4, 256, device="cuda", dtype=torch.bfloat16), torch.zeros(4, 256, device="cuda", dtype=torch.bfloat16), 4)
