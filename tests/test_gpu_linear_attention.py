"""svdq_linear_attention on the GPU: SANA's ReLU linear attention over the packed QKV buffer, against the fp64 restatement of
tests/litela_ref.py on the same 16-bit inputs.

Gates on ``out`` (the attention gates of tests/test_gpu_ip_attention.py): |err| <= 3 * 2^-8 (bf16) / 3 * 2^-11 (fp16) relative to
max|ref|, and no worse than 1.5 x the error of the fp32 restatement rounded once (+ 1e-6).  Gate on ``vk``, elementwise:
|vk - vk64| <= T * 2^-23 * sum_t |V[t, i]| relu(K[t, j]) (row 32: |V| replaced by 1) -- the first-order bound of an fp32 sum of T exactly
representable products in any order, times 2 because the order inside the matrix core is unspecified.  Derived, not measured."""

import functools

import pytest
import torch
import torch.nn.functional as F

from tests.litela_ref import litela_16bit, litela_ref32, litela_ref64, split_qkv

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SHAPES = [(1, 1, 1), (1, 31, 3), (2, 256, 2), (3, 300, 5), (1, 1030, 36), (2, 2100, 4)]  # (B, T, H); the kernel's token chunk is 256
DTYPES = ["bf16", "fp16"]


@functools.lru_cache(maxsize=None)
def _case(B, T, H, dtype):
    """packed qkv [B, T, 3*H*32] on the CPU (randn; the Q columns of the first half of the rows x 4) and its references, computed once"""
    g = torch.Generator().manual_seed(100000 * B + 10 * T + H)
    qkv = torch.randn(B, T, 3 * H * 32, generator=g).to(TD[dtype])
    qkv[:, : T // 2, : H * 32] *= 4.0
    out64, vk64 = litela_ref64(qkv, H)
    return qkv, out64, vk64, litela_ref32(qkv, H)[0]


def _gate_out(out, qkv, H, dtype, what, second_gate=True, refs=None):
    """``refs``: (fp64 reference, fp32 restatement rounded once) when the caller has them already"""
    out64, out32 = refs if refs is not None else (litela_ref64(qkv, H)[0], litela_ref32(qkv, H)[0])
    err = (out.cpu().double() - out64).abs().max().item()
    err32 = (out32.double() - out64).abs().max().item()
    err16 = (litela_16bit(qkv.cuda(), H).cpu().double() - out64).abs().max().item()
    tol = 3 * ULP[dtype] * out64.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), fp32 restatement rounded once {err32:.3g}, all-16-bit torch ops {err16:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g}"
    if second_gate:
        assert err <= 1.5 * err32 + 1e-6, f"{what}: error {err:.3g} vs the fp32 restatement's {err32:.3g}"


def _gate_vk(vk, qkv, H, what):
    """qkv: the 16-bit values the sums run over, [B, T, 3*H*32]"""
    T = qkv.shape[1]
    _, k, v = (t.double() for t in split_qkv(qkv.cpu(), H))
    rk = torch.relu(k)
    vk64 = torch.cat([torch.einsum("bthi,bthj->bhij", v, rk), rk.sum(dim=1)[:, :, None, :]], dim=2)
    bound = T * 2.0 ** -23 * torch.cat([torch.einsum("bthi,bthj->bhij", v.abs(), rk), rk.sum(dim=1)[:, :, None, :]], dim=2)
    err = (vk.cpu().double() - vk64).abs()
    used = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: vk error uses {used:.3g} of its bound (max |vk| {vk64.abs().max().item():.4g})")
    assert vk.dtype == torch.float32 and tuple(vk.shape) == tuple(vk64.shape)
    assert (err <= bound).all(), f"{what}: vk off by {used:.3g} x its bound"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_accuracy_of_out_and_vk(B, T, H, dtype):
    from nunchaku_amd.ops.attention import linear_attention

    qkv, out64, _, out32 = _case(B, T, H, dtype)
    out, vk = linear_attention(qkv.cuda(), H, return_vk=True)
    assert out.shape == (B, T, H * 32) and out.dtype == TD[dtype]
    _gate_out(out, qkv, H, dtype, f"({B},{T},{H}) {dtype}", refs=(out64, out32))
    _gate_vk(vk, qkv, H, f"({B},{T},{H}) {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_calls_are_bit_equal(B, T, H, dtype):
    """in the default mode: no atomics anywhere, the chunks' partials are added in chunk order"""
    from nunchaku_amd.ops.attention import linear_attention

    dev = _case(B, T, H, dtype)[0].cuda()
    out, vk = linear_attention(dev, H, return_vk=True)
    again, vk_again = linear_attention(dev, H, return_vk=True)
    assert torch.equal(out, again) and torch.equal(vk, vk_again)
    assert torch.equal(linear_attention(dev, H), out)  # with and without vk
    flat = linear_attention(dev.view(B * T, -1), H, tokens=T)
    assert flat.shape == (B * T, H * 32) and torch.equal(flat.view(B, T, -1), out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_nothing_outside_the_operands_is_read_or_written(B, T, H, dtype):
    """The packed buffer sits in a larger NaN-filled one (a larger batch stride, extra columns on the right: the rows at and beyond T of every
    batch element are NaN and batch elements do not start on a 256-row boundary); out is a column slice of a sentinel-filled buffer."""
    from nunchaku_amd.ops.attention import linear_attention

    qkv = _case(B, T, H, dtype)[0].cuda()
    W, hd = 3 * H * 32, H * 32
    clean, vk_clean = linear_attention(qkv, H, return_vk=True)
    big = torch.full((B, T + 40, W + 64), float("nan"), device="cuda", dtype=TD[dtype])
    big[:, :T, :W] = qkv
    sentinel = -77.0
    big_o = torch.full((B, T + 33, hd + 128), sentinel, device="cuda", dtype=TD[dtype])
    out = big_o[:, :T, 64:64 + hd]
    got, vk = linear_attention(big[:, :T, :W], H, out=out, return_vk=True)
    assert got is out and torch.isfinite(out).all() and torch.equal(out, clean) and torch.equal(vk, vk_clean)
    assert (big_o[:, T:] == sentinel).all() and (big_o[:, :T, :64] == sentinel).all() and (big_o[:, :T, 64 + hd:] == sentinel).all()
    assert torch.isnan(big[:, T:]).all() and torch.isnan(big[:, :, W:]).all() and torch.equal(big[:, :T, :W], qkv)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_without_positive_q_and_heads_without_positive_k_give_exact_zeros(dtype):
    from nunchaku_amd.ops.attention import linear_attention

    B, T, H = 2, 300, 5
    qkv = _case(3, T, H, dtype)[0][:B].clone()
    hd = H * 32
    qkv[0, 7, :hd] = -qkv[0, 7, :hd].abs()           # Q <= 0 in every head of one row
    qkv[1, 299, 32:64] = -qkv[1, 299, 32:64].abs()   # ... and in one head of the last row
    qkv[1, 299, 40] = 0.0
    ks = hd + 64 * 3                                 # K of head 3
    qkv[1, :, ks: ks + 32] = -qkv[1, :, ks: ks + 32].abs()
    qkv[1, 11, ks + 5] = 0.0
    out, vk = linear_attention(qkv.cuda(), H, return_vk=True)
    assert torch.isfinite(out).all()                 # (0 / eps, not 0 / 0)
    assert (out[0, 7] == 0).all() and (out[1, 299, 32:64] == 0).all() and (out[1, :, 96:128] == 0).all() and (vk[1, 3] == 0).all()
    assert (out[0, 6] != 0).any() and (out[1, 299, :32] != 0).any() and (out[0, :, 96:128] != 0).any()
    _gate_out(out, qkv, H, dtype, f"zero rows and a zero head {dtype}")
    _gate_vk(vk, qkv, H, f"zero rows and a zero head {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H", [(1, 1), (3, 7)])
def test_a_single_token_returns_its_v_row(B, H, dtype):
    """T = 1: out = v * s / (s + eps) with s = relu(q) . relu(k): the V row bit for bit wherever s > 2^-10"""
    from nunchaku_amd.ops.attention import linear_attention

    g = torch.Generator().manual_seed(17 + H)
    qkv = torch.randn(B, 1, 3 * H * 32, generator=g).to(TD[dtype])
    q, k, v = split_qkv(qkv, H)
    s = (torch.relu(q.double()) * torch.relu(k.double())).sum(-1)  # [B, 1, H]
    live = s > 2.0 ** -10
    assert live.any()
    out = linear_attention(qkv.cuda(), H).cpu().view(B, 1, H, 32)
    assert torch.equal(out[live], v[live])


def test_fp16_sums_far_beyond_the_format_stay_finite():
    """|values| around 200 over T = 2100: the sums of products of random sign reach 200 * 200 * sqrt(1050) ~ 1e6, far beyond 65504 -- fp32 all the
    way to the quotient"""
    from nunchaku_amd.ops.attention import linear_attention

    B, T, H = 1, 2100, 2
    g = torch.Generator().manual_seed(5)
    mag = (torch.rand(B, T, 3 * H * 32, generator=g) * 0.5 + 0.75) * 200.0
    qkv = (mag * torch.sign(torch.randn(B, T, 3 * H * 32, generator=g))).to(torch.float16)
    out, vk = linear_attention(qkv.cuda(), H, return_vk=True)
    assert vk.abs().max().item() > 65504 * 4
    _gate_out(out, qkv, H, "fp16", "fp16, magnitude 200, T = 2100", second_gate=False)
    _gate_vk(vk, qkv, H, "fp16, magnitude 200, T = 2100")


def test_wrapper_checks_on_gpu_tensors():
    from nunchaku_amd._C import ops

    qkv = torch.zeros(2, 8, 3 * 2 * 32, device="cuda", dtype=torch.bfloat16)
    q, kv = qkv[..., :64].unflatten(-1, (2, 32)), qkv[..., 64:].unflatten(-1, (2, 64))
    with pytest.raises(ValueError, match="one 16-bit dtype"):
        ops.linear_attention(q, kv, torch.zeros(2, 8, 2, 32, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError, match="vk must be"):
        ops.linear_attention(q, kv, torch.zeros_like(q), vk=torch.zeros(2, 2, 32, 32, device="cuda"))
    with pytest.raises(NotImplementedError, match="head_dim=64"):
        ops.linear_attention(qkv[..., :64].unflatten(-1, (1, 64)), qkv[..., 64:].unflatten(-1, (1, 128)), torch.zeros(2, 8, 1, 64, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 8"):  # rows that are not 16-byte aligned
        odd = torch.zeros(2, 8, 3 * 64 + 4, device="cuda", dtype=torch.bfloat16)
        ops.linear_attention(odd[..., :64].unflatten(-1, (2, 32)), odd[..., 64:192].unflatten(-1, (2, 64)), torch.zeros_like(q))


@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


def _layer(K, N, seed, dtype="bf16", prefix=""):
    from oracle import svdq_oracle as O
    from tests.helpers import reference_state_dict

    L = O.make_svdq_layer(K, N, 32, seed=seed, dtype=dtype, bias=False, cheap=True)
    return L, {prefix + k: v for k, v in reference_state_dict(L, dtype).items()}


def test_gemm_w4a4_honours_out_vk_and_out_linearattn(strict_mode):
    """the reference's LiteLA contract (gemm_w4a4_launch_impl.cuh:311-345) as a compatibility path: the plain epilogue into a scratch, relu(Q) into
    out_linearattn, the sums over ALL T_pad rows of every batch element into out_vk"""
    from oracle import svdq_oracle as O
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda
    from tests.helpers import make_module, t16

    K, N, Bc, T_pad = 256, 3 * 2 * 32 * 2, 2, 256
    Hc = N // 96
    assert N % 384 == 0 and N % 128 == 0
    mod = make_module(_layer(K, N, seed=3)[0], "bf16")
    x = t16(O.make_activations(Bc * T_pad, K, seed=3), "bf16")
    qx, asc, la = mod.quantize(x)
    kw = dict(act=qx, wgt=mod.qweight, ascales=asc, wscales=mod.wscales, lora_act_in=la, lora_up=mod.proj_up, bias=mod.bias,
              act_unsigned=mod.act_unsigned)
    plain = torch.empty(Bc * T_pad, N, device="cuda", dtype=torch.bfloat16)
    svdq_gemm_w4a4_cuda(out=plain, **kw)
    o_q = torch.full((Bc, T_pad, N // 3), float("nan"), device="cuda", dtype=torch.bfloat16)
    o_vk = torch.full((Bc, Hc, 33, 32), float("nan"), device="cuda")
    svdq_gemm_w4a4_cuda(out_vk=o_vk, out_linearattn=o_q, **kw)
    packed = plain.view(Bc, T_pad, N)
    assert torch.equal(o_q, torch.relu(packed[..., : N // 3]))
    _gate_vk(o_vk, packed, Hc, "gemm_w4a4(out_vk=, out_linearattn=)")
    assert (o_vk[:, :, 32] > 0).all()

    vk = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="cuda", dtype=dtype)
    lin = lambda *shape: torch.empty(*shape, device="cuda", dtype=torch.bfloat16)
    for bad in (dict(out_vk=o_vk), dict(out_linearattn=o_q),                                    # one without the other
                dict(out_vk=vk(Bc, Hc, 32, 32), out_linearattn=o_q),                             # launch_impl.cuh:319
                dict(out_vk=vk(Bc, Hc, 33, 64), out_linearattn=o_q),                             # :320
                dict(out_vk=vk(Bc, Hc + 1, 33, 32), out_linearattn=o_q),                         # :321
                dict(out_vk=vk(Bc, Hc, 33, 32, dtype=torch.float64), out_linearattn=o_q),        # :317
                dict(out_vk=vk(Bc * Hc, 33, 32), out_linearattn=o_q),                            # :318
                dict(out_vk=o_vk, out_linearattn=lin(Bc + 1, T_pad, N // 3)),                    # :327
                dict(out_vk=o_vk, out_linearattn=lin(Bc, T_pad, N // 3 + 32)),                   # :328
                dict(out_vk=o_vk, out_linearattn=lin(Bc * T_pad, N // 3)),                       # :326
                dict(out_vk=o_vk, out_linearattn=lin(Bc, 300, N // 3)),                          # :331, T_pad % 256
                dict(out_vk=o_vk, out_linearattn=o_q, out=plain)):                               # the epilogue has no other output
        with pytest.raises(ValueError):
            svdq_gemm_w4a4_cuda(**{**kw, **bad})


@pytest.mark.parametrize("dim", [256, 320])
def test_module_equals_its_composition_from_the_public_pieces(dim, strict_mode):
    from nunchaku_amd.models import SanaLinearAttention
    from nunchaku_amd.ops.attention import linear_attention

    B, T = 2, 300
    m = SanaLinearAttention(dim, pag=True, device="cuda")
    dp = m.dim_pad
    assert dp == (256 if dim == 256 else 384) and m.heads == dp // 32
    sd = {}
    for i, (name, n_out) in enumerate((("qkv_proj", 3 * dp), ("out_proj", dp), ("pag_to_v", dp))):
        sd.update(_layer(dp, n_out, seed=10 + i, prefix=name + ".")[1])
    m.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(3, T, dim, generator=g).to(torch.bfloat16).cuda()
    pad = lambda t: F.pad(t, (0, dp - dim))

    y = m(x[:B])
    qkv = m.qkv_proj(pad(x[:B]))
    attn = linear_attention(qkv, m.heads)
    hand = m.out_proj(attn)[..., :dim]
    assert y.shape == (B, T, dim) and torch.isfinite(y).all() and torch.equal(y, hand)
    assert torch.equal(m(x[:B]), y)                              # a second call
    into = torch.full((B, T, dim), float("nan"), device="cuda", dtype=torch.bfloat16)
    assert m(x[:B], out=into) is into and torch.equal(into, y)
    _gate_out(attn, qkv.cpu(), m.heads, "bf16", f"dim {dim}: the attention inside the module")  # accuracy is the op's, on the module's own QKV

    ptb = lambda t: m.out_proj(m.pag_to_v(pad(t)))[..., :dim]
    assert torch.equal(m.forward_pag(x[:B], False), torch.cat([m(x[:1]), ptb(x[1:2])]))
    assert torch.equal(m.forward_pag(x, True), torch.cat([m(x[:2]), ptb(x[2:])]))
    with pytest.raises(ValueError):
        m.forward_pag(x, False)
