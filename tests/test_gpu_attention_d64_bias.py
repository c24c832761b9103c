"""svdq_attention_d64_bias against float64 (tests/attention_d64_bias_ref.py).  The gate is tests/test_gpu_attention_d64.py's: |err| <= 3 * 2^-8 (bf16) /
3 * 2^-11 (fp16) of max|ref|, and <= 1.5 x the 16-bit eager sequence's error + 1e-6.  Tile 128 rows, chunk 64 keys: shapes around both edges, T != N both ways."""

import pytest
import torch

from tests.attention_d64_bias_ref import attention_d64_bias_ref, eager16_d64_bias

pytestmark = pytest.mark.gpu

TD, ULP, DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}, {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}, ["bf16", "fp16"]
CASES = [(1, 1, 1, 1), (2, 127, 2, 63), (1, 128, 1, 64), (2, 129, 2, 65), (1, 257, 1, 128), (2, 300, 2, 300), (1, 40, 3, 200), (1, 200, 2, 40)]  # (B, T, H, N)
NAN, INF = float("nan"), float("inf")


def _inputs(B, T, H, N, dtype, seed=0):  # q [B, T, H*64] (half the rows x 4: peaky), k, v [B, N, H*64], rel_bias [H, T + N - 1] = 2 x normal
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + N)
    q, k, v = (torch.randn(B, rows, H * 64, device="cuda", generator=g).to(TD[dtype]) for rows in (T, N, N))
    q[:, : T // 2] *= 4.0
    return q, k, v, 2.0 * torch.randn(H, T + N - 1, device="cuda", generator=g)


def _excluding(B, N, value):  # key_bias [B, N]: 0, and `value` on each sample's last N // 3 keys
    return torch.cat((torch.zeros(B, N - N // 3, device="cuda"), torch.full((B, N // 3), value, device="cuda")), dim=1)


def _gate(out, q, k, v, H, rel, kb, dtype, what):
    ref = attention_d64_bias_ref(q, k, v, H, rel, kb)
    err = (out.double() - ref).abs().max().item()
    err_eager = (eager16_d64_bias(q, k, v, H, rel, kb).double() - ref).abs().max().item()
    tol = 3 * ULP[dtype] * ref.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), 16-bit eager sequence {err_eager:.3g}")
    assert torch.isfinite(out).all() and err <= tol and err <= 1.5 * err_eager + 1e-6, f"{what}: error {err:.3g}, gate {tol:.3g}, eager {err_eager:.3g}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
@pytest.mark.parametrize("B,T,H,N", CASES, ids=[f"B{B}-T{T}-H{H}-N{N}" for B, T, H, N in CASES])
def test_accuracy_two_launches_packed_form_and_per_sample_equality(B, T, H, N, masked, dtype):
    from nunchaku_amd.ops import attention_d64_bias

    hd = H * 64
    q, k, v, rel = _inputs(B, T, H, N, dtype)
    kb = _excluding(B, N, torch.finfo(TD[dtype]).min) if masked else None
    out = attention_d64_bias(q, k, v, H, rel, kb)
    assert out.shape == (B, T, hd) and out.dtype == TD[dtype] and out.is_contiguous()
    _gate(out, q, k, v, H, rel, kb, dtype, f"({B},{T},{H},{N}) {dtype} masked={masked}")
    assert torch.equal(attention_d64_bias(q, k, v, H, rel, kb, out=torch.empty_like(out)), out)  # two launches
    if T == N:  # the packed form: q, k, v as the thirds of one [B, T, 3 * H * 64] buffer
        qkv = torch.cat((q, k, v), dim=-1)
        assert torch.equal(attention_d64_bias(qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:], H, rel, kb), out)
    for b in range(B):  # every sample alone, its tensors cloned
        one = attention_d64_bias(q[b].clone(), k[b].clone(), v[b].clone(), H, rel, None if kb is None else kb[b:b + 1].clone())
        assert torch.equal(one, out[b]), f"sample {b}"
    if T == N == 300 and not masked:  # rel_bias from T5's own bucket function over -299 .. 299 (beyond +-128 it saturates) and a random [32, H] table
        from transformers.models.t5.modeling_t5 import T5Attention

        rel = rel[:, :32].t()[T5Attention._relative_position_bucket(torch.arange(-(T - 1), N, device="cuda"))].t().contiguous()
        _gate(attention_d64_bias(q, k, v, H, rel), q, k, v, H, rel, None, dtype, f"T5 buckets {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [-129, -65, -64, -1, 0, 1, 63, 64, 129])
def test_the_toeplitz_index_bit_for_bit(d, dtype):
    """q = 0, rel_bias 0 on ONE diagonal and -100 elsewhere (e^-100 of weight per other key): row t returns v[t + d] bit for bit; head 1 takes -d"""
    from nunchaku_amd.ops import attention_d64_bias

    T, H = 300, 2
    v = torch.randn(1, T, H * 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(300 + d)).to(TD[dtype])
    rel = torch.full((H, 2 * T - 1), -100.0, device="cuda")
    rel[0, d + T - 1] = rel[1, -d + T - 1] = 0.0
    out = attention_d64_bias(torch.zeros_like(v), torch.zeros_like(v), v, H, rel)
    compared = 0
    for h, dh in ((0, d), (1, -d)):
        t = torch.arange(max(0, -dh), min(T, T - dh), device="cuda")
        assert torch.equal(out[0, t, 64 * h:64 * h + 64], v[0, t + dh, 64 * h:64 * h + 64]), f"head {h}, diagonal {dh}"
        compared += t.numel()
    assert compared >= T  # at least half of the 2 x 300 rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_exclusion_contract(dtype):
    from nunchaku_amd.ops import attention_d64_bias

    B, T, H, N = 2, 130, 2, 200
    q, k, v, rel = _inputs(B, T, H, N, dtype, seed=2)
    kb = _excluding(B, N, -INF)
    out = attention_d64_bias(q, k, v, H, rel, kb)
    assert torch.equal(attention_d64_bias(q, k, v, H, rel, _excluding(B, N, torch.finfo(torch.bfloat16).min)), out)
    # keys 134 .. 199 are excluded: keys 192 .. 199 share their 64-key chunk with keys beyond N only, and NaN there changes nothing
    kn, vn = (torch.cat((t[:, :192], torch.full_like(t[:, 192:], NAN)), dim=1) for t in (k, v))
    assert torch.equal(attention_d64_bias(q, kn, vn, H, rel, kb), out)
    kb[1] = -INF  # a sample with every key excluded: exact zeros, the other sample as before
    got = attention_d64_bias(q, k, v, H, rel, kb)
    assert torch.equal(got[0], out[0]) and (got[1] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,N", [(2, 48, 3, 77), (1, 129, 2, 65)], ids=["B2-T48-H3-N77", "B1-T129-H2-N65"])
def test_nothing_outside_the_operands_is_read_or_written(B, T, H, N, dtype):
    """test_gpu_attention_d64.py's NaN frames around q, k, v, out; rel_bias and key_bias are the middles of NaN-framed buffers (a window load off either end)"""
    from nunchaku_amd.ops import attention_d64_bias

    hd, td = H * 64, TD[dtype]
    q, k, v, rel = _inputs(B, T, H, N, dtype, seed=3)
    kb = _excluding(B, N, -3.0)
    clean = attention_d64_bias(q, k, v, H, rel, kb)
    qb = torch.full((B, T + 5, hd + 128), NAN, device="cuda", dtype=td)
    qb[:, :T, 64:64 + hd] = q
    kf, vf = (torch.full((B, N + 7, hd + 64), NAN, device="cuda", dtype=td) for _ in range(2))
    kf[:, :N, :hd], vf[:, :N, :hd] = k, v
    vf[:, N:, :hd] = 6e4
    relf, kbf = (torch.full((t.numel() + 512,), NAN, device="cuda") for t in (rel, kb))
    relf[256:-256], kbf[256:-256] = rel.flatten(), kb.flatten()
    ob = torch.full((B, T + 3, hd + 128), 7.0, device="cuda", dtype=td)
    got = attention_d64_bias(qb[:, :T, 64:64 + hd], kf[:, :N, :hd], vf[:, :N, :hd], H, relf[256:-256].view(H, -1), kbf[256:-256].view(B, N),
                             out=ob[:, :T, 64:64 + hd])
    assert got.data_ptr() == ob[:, :T, 64:64 + hd].data_ptr() and torch.equal(got, clean)
    assert (ob[:, T:] == 7.0).all() and (ob[:, :, :64] == 7.0).all() and (ob[:, :, 64 + hd:] == 7.0).all()


def test_op_errors():
    from nunchaku_amd.ops import attention_d64_bias

    q, k, v, rel = _inputs(2, 16, 2, 20, "bf16")
    kb = torch.zeros(2, 20, device="cuda")
    for bad in (rel[:, :-1], rel.double(), rel.cpu(), torch.zeros(2, 2 * 35, device="cuda")[:, ::2], kb[:, :19]):  # length, dtype, device, strides; key_bias
        with pytest.raises(ValueError, match="(rel|key)_bias must"):
            attention_d64_bias(q, k, v, 2, *((rel, bad) if bad.shape[1] == 19 else (bad, kb)))
    with pytest.raises(NotImplementedError, match="head_dim=128"):
        attention_d64_bias(q, k, v, 1, rel[:1], kb)
    with pytest.raises(ValueError, match="out overlaps q"):
        attention_d64_bias(q, k, v, 2, rel, kb, out=q)


def test_the_call_can_be_captured_in_a_graph():
    from nunchaku_amd.ops import attention_d64_bias

    q, k, v, rel = _inputs(2, 130, 2, 77, "bf16", seed=9)
    kb = _excluding(2, 77, -INF)
    want = attention_d64_bias(q, k, v, 2, rel, kb)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        attention_d64_bias(q, k, v, 2, rel, kb, out=out)
    graph.replay()
    assert torch.equal(out, want)
