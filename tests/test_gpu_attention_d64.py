"""svdq_attention_d64 on the GPU: Stable Diffusion XL's attention at head dimension 64 (batched, K and V streamed in 64-key chunks, Q / K / V read
in place from the thirds of a packed QKV projection or from separate projections) against the fp32 restatement of tests/attention_d64_ref.py.
The accuracy gate is the one of tests/test_gpu_cross_attention.py: |err| <= 3 * 2^-8 (bf16) / 3 * 2^-11 (fp16) relative to max|ref|, and no
worse than 1.5 x the error of torch's own 16-bit SDPA on the same inputs (+ 1e-6); half of the query rows are scaled by 4 so that some
softmaxes are peaky.  The query tile is 128 rows (T = 127 / 128 / 129 sit below, at and above its edge; 257 and 300 take three tiles) and the
key chunk 64 (N = 63 / 64 / 65 / 128 / 129; 77 is SDXL's text length)."""

import pytest
import torch

from tests.attention_d64_ref import attention_d64_ref, sdpa16_d64

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DTYPES = ["bf16", "fp16"]
CASES = [  # (B, T, H, N)
    (1, 1, 1, 1),
    (2, 48, 3, 77),
    (1, 127, 2, 63),
    (2, 128, 1, 64),
    (1, 129, 2, 65),
    (2, 257, 1, 128),
    (1, 40, 10, 129),
    (2, 300, 2, 300),
    (1, 64, 20, 520),
]
IDS = [f"B{B}-T{T}-H{H}-N{N}" for B, T, H, N in CASES]
SMALL = [(2, 48, 3, 77), (1, 129, 2, 65), (2, 128, 1, 64)]
SMALL_IDS = [f"B{B}-T{T}-H{H}-N{N}" for B, T, H, N in SMALL]
NAN = float("nan")


def _inputs(B, T, H, N, dtype, seed=0):
    """q [B, T, H*64] (half the query rows x 4: peaky rows) and k, v [B, N, H*64], each contiguous"""
    hd = H * 64
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + N)
    q = torch.randn(B, T, hd, device="cuda", generator=g).to(TD[dtype])
    q[:, : T // 2] *= 4.0
    k = torch.randn(B, N, hd, device="cuda", generator=g).to(TD[dtype])
    v = torch.randn(B, N, hd, device="cuda", generator=g).to(TD[dtype])
    return q, k, v


def _gate(out, q, k, v, H, dtype, what=""):
    ref = attention_d64_ref(q, k, v, H)
    err = (out.float() - ref).abs().max().item()
    err_sdpa = (sdpa16_d64(q, k, v, H).float() - ref).abs().max().item()
    tol = 3 * ULP[dtype] * ref.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), torch 16-bit SDPA {err_sdpa:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g}"
    assert err <= 1.5 * err_sdpa + 1e-6, f"{what}: error {err:.3g} vs torch 16-bit SDPA {err_sdpa:.3g}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,N", CASES, ids=IDS)
def test_accuracy_two_launches_packed_form_and_per_sample_equality(B, T, H, N, dtype):
    from nunchaku_amd.ops import attention_d64

    hd = H * 64
    q, k, v = _inputs(B, T, H, N, dtype)
    out = attention_d64(q, k, v, H)
    assert out.shape == (B, T, hd) and out.dtype == TD[dtype] and out.is_contiguous()
    _gate(out, q, k, v, H, dtype, f"({B},{T},{H},{N}) {dtype}")
    assert torch.equal(attention_d64(q, k, v, H), out)                                   # two launches
    assert torch.equal(attention_d64(q, k, v, H, scale=0.125, out=torch.empty_like(out)), out)
    # the packed self-attention form: q, k, v as the thirds of one [B, S, 3 * H * 64] buffer (S = T = N) against three contiguous tensors
    S = T
    g = torch.Generator(device="cuda").manual_seed(7 + S + H)
    qkv = torch.randn(B, S, 3 * hd, device="cuda", generator=g).to(TD[dtype])
    qkv[:, : S // 2, :hd] *= 4.0
    packed = attention_d64(qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:], H)
    qc, kc, vc = (t.contiguous() for t in qkv.chunk(3, dim=-1))
    apart = attention_d64(qc, kc, vc, H)
    assert torch.equal(packed, apart)
    _gate(packed, qc, kc, vc, H, dtype, f"packed ({B},{S},{H},{S}) {dtype}")
    # every sample alone (3-D with B = 1, and 2-D), its tensors cloned
    for b in range(B):
        one = attention_d64(q[b:b + 1].clone(), k[b:b + 1].clone(), v[b:b + 1].clone(), H)
        assert torch.equal(one[0], out[b]), f"sample {b}"
        flat = attention_d64(q[b].clone(), k[b].clone(), v[b].clone(), H)
        assert flat.shape == (T, hd) and torch.equal(flat, out[b]), f"sample {b}, 2-D"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,N", SMALL, ids=SMALL_IDS)
def test_nothing_outside_the_operands_is_read_or_written(B, T, H, N, dtype):
    from nunchaku_amd.ops import attention_d64

    hd, td = H * 64, TD[dtype]
    q, k, v = _inputs(B, T, H, N, dtype, seed=3)
    clean = attention_d64(q, k, v, H)
    # q: NaN in 64 extra columns on either side and in 5 rows behind each sample's T
    qb = torch.full((B, T + 5, hd + 128), NAN, device="cuda", dtype=td)
    qb[:, :T, 64:64 + hd] = q
    # k / v: NaN (K) and 6e4 (V) in the 7 rows behind each sample's N keys; NaN in the columns beyond H * 64
    kb = torch.full((B, N + 7, hd + 64), NAN, device="cuda", dtype=td)
    vb = torch.full((B, N + 7, hd + 64), NAN, device="cuda", dtype=td)
    kb[:, :N, :hd] = k
    vb[:, :N, :hd] = v
    vb[:, N:, :hd] = 6e4
    # out: a column slice of a sentinel-filled larger buffer
    ob = torch.full((B, T + 3, hd + 128), 7.0, device="cuda", dtype=td)
    got = attention_d64(qb[:, :T, 64:64 + hd], kb[:, :N, :hd], vb[:, :N, :hd], H, out=ob[:, :T, 64:64 + hd])
    assert got.data_ptr() == ob[:, :T, 64:64 + hd].data_ptr() and torch.equal(got, clean)
    assert (ob[:, T:] == 7.0).all() and (ob[:, :, :64] == 7.0).all() and (ob[:, :, 64 + hd:] == 7.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,H,N", [(40, 2, 65), (129, 1, 200), (33, 3, 64)])
def test_a_dominant_key_returns_its_v_row_exactly(T, H, N, dtype):
    """a row whose score for one key exceeds every other by more than 40 (in scaled units: exp(-40) = 4e-18 of weight for each other key, far
    below half an ulp of the 16-bit result and of the fp32 row sum) returns that key's V row bit for bit -- wherever the key sits: first, on
    either side of a chunk edge, last"""
    from nunchaku_amd.ops import attention_d64

    hd, td = H * 64, TD[dtype]
    g = torch.Generator(device="cuda").manual_seed(N + T)
    v = torch.randn(1, N, hd, device="cuda", generator=g).to(td)
    for star in sorted({0, 63, min(64, N - 1), N - 1}):
        # q . k = 64 * 2 * 4 = 512 for the star key (scaled: 64), 64 * 2 * (+-0.5) = +-64 for the others (scaled: at most 8)
        q = torch.full((1, T, hd), 2.0, device="cuda", dtype=td)
        k = (torch.randint(0, 2, (1, N, hd), device="cuda", generator=g).to(td) - 0.5)
        k[0, star] = 4.0
        out = attention_d64(q, k, v, H)
        assert torch.equal(out, v[:, star:star + 1].expand(1, T, hd)), f"star key {star} of {N}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,N", [(2, 48, 3, 77), (3, 130, 2, 129)], ids=["B2-T48-H3-N77", "B3-T130-H2-N129"])
def test_a_sample_sees_its_own_keys_only(B, T, H, N, dtype):
    from nunchaku_amd.ops import attention_d64

    q, k, v = _inputs(B, T, H, N, dtype, seed=5)
    clean = attention_d64(q, k, v, H)
    for b in range(B):
        kk, vv = k.clone(), v.clone()
        other = (b + 1) % B
        kk[other], vv[other] = NAN, NAN
        got = attention_d64(q, kk, vv, H)
        assert torch.equal(got[b], clean[b]), f"sample {b} changed when sample {other}'s keys did"
        assert torch.isnan(got[other]).all()
    # and its own head's: NaN in every other head's K / V columns
    if H > 1:
        kk, vv = k.clone(), v.clone()
        kk[..., 64:], vv[..., 64:] = NAN, NAN
        assert torch.equal(attention_d64(q, kk, vv, H)[..., :64], clean[..., :64])


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_errors(dtype):
    from nunchaku_amd.ops import attention_d64

    td = TD[dtype]
    q, k, v = _inputs(2, 16, 2, 20, dtype)
    with pytest.raises(NotImplementedError, match="head_dim=128"):
        attention_d64(q, k, v, 1)
    with pytest.raises(NotImplementedError, match="head_dim=32"):
        attention_d64(q, k, v, 4)
    wide = torch.zeros(2, 16, 128 + 4, device="cuda", dtype=td)
    with pytest.raises(ValueError, match="16-byte aligned"):                      # a row stride of 132 elements
        attention_d64(wide[..., :128], k, v, 2)
    with pytest.raises(ValueError, match="16-byte aligned"):                      # a pointer 8 bytes into a row
        attention_d64(torch.zeros(2, 16, 136, device="cuda", dtype=td)[..., 4:132], k, v, 2)
    with pytest.raises(ValueError, match="heads D elements apart|unit channel stride"):
        attention_d64(torch.zeros(2, 16, 256, device="cuda", dtype=td)[..., ::2], k, v, 2)
    odd = torch.zeros(2 * 16 * 128 + 4, device="cuda", dtype=td)
    with pytest.raises(ValueError, match="must be a multiple of 8"):              # samples 16 * 128 + 4 elements apart
        attention_d64(odd.as_strided((2, 16, 128), (16 * 128 + 4, 128, 1)), k, v, 2)
    with pytest.raises(ValueError, match="out overlaps q"):
        attention_d64(q, k, v, 2, out=q)
    kv = torch.zeros(2, 20, 256, device="cuda", dtype=td)
    with pytest.raises(ValueError, match="out overlaps k"):                       # out: the other half of k's rows
        attention_d64(q, kv[..., 128:], v, 2, out=kv[:, :16, :128])
    with pytest.raises(ValueError, match="scale must be positive and finite"):
        attention_d64(q, k, v, 2, scale=0.0)
    # an expanded K / V (one text condition for both samples) is a stride the kernel takes only as B separate buffers: refused, not misread
    with pytest.raises(ValueError, match="batch strides"):
        attention_d64(q, k[:1].expand(2, 20, 128), v[:1].expand(2, 20, 128), 2)


def test_the_call_can_be_captured_in_a_graph():
    from nunchaku_amd.ops import attention_d64

    q, k, v = _inputs(2, 130, 2, 77, "bf16", seed=9)
    want = attention_d64(q, k, v, 2)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        attention_d64(q, k, v, 2, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
