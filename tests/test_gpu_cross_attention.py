"""svdq_cross_attention on the GPU: SANA's text cross-attention (thousands of queries per sample against that sample's range of at most 320 keys,
Q read in place from q_linear's padded rows, K / V from the two column halves of kv_linear's output, the ranges read on the device) against
the fp32 restatement of tests/xattn_ref.py.  The accuracy gate is the one of tests/test_gpu_attention.py and tests/test_gpu_ip_attention.py:
|err| <= 3 * 2^-8 (bf16) / 3 * 2^-11 (fp16) relative to max|ref|, and no worse than 1.5 x the error of torch's own 16-bit SDPA run per
sample on the same inputs.  The kernel walks a sample's keys in chunks of 64: the counts 127 / 128 / 65 / 64 / 33 / 300 / 320 sit below, at
and above chunk edges."""

import pytest
import torch
import torch.nn.functional as F

from tests.xattn_ref import clamp_ranges, sdpa16, xattn_ref

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DTYPES = ["bf16", "fp16"]
CASES = [  # (B, T, H, D, counts)
    (1, 16, 1, 128, [1]),
    (2, 48, 3, 112, [4, 37]),
    (3, 300, 2, 72, [300, 0, 65]),
    (2, 257, 1, 112, [33, 300]),
    (2, 64, 20, 112, [127, 128]),
    (3, 40, 16, 72, [1, 300, 64]),
    (1, 520, 2, 128, [320]),
]
IDS = [f"B{B}-T{T}-H{H}-D{D}-" + "_".join(map(str, c)) for B, T, H, D, c in CASES]
NAN = float("nan")


def _ceil128(n):
    return (n + 127) // 128 * 128


def _cu(counts):
    return torch.tensor([sum(counts[:b]) for b in range(len(counts) + 1)], dtype=torch.int32, device="cuda")


def _offsets(counts):
    return [sum(counts[:b]) for b in range(len(counts))]


def _inputs(B, T, H, D, counts, dtype, seed=0):
    """q [B, T, ceil128(H*D)] as q_linear writes it (half the query rows x 4: peaky rows; the columns beyond H*D hold numbers too) and the
    packed kv [sum(counts), 2*H*D] of kv_linear -> q, kv, k, v (k and v: the column halves of kv, no copy)"""
    hd = H * D
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + D + sum(counts))
    q = torch.randn(B, T, _ceil128(hd), device="cuda", generator=g).to(TD[dtype])
    q[:, : T // 2] *= 4.0
    kv = torch.randn(max(sum(counts), 1), 2 * hd, device="cuda", generator=g).to(TD[dtype])[: sum(counts)]
    return q, kv, kv[:, :hd], kv[:, hd:]


def _gate(out, q, k, v, H, D, offs, counts, dtype, what=""):
    ref = xattn_ref(q, k, v, H, D, offs, counts)
    err = (out.float() - ref).abs().max().item()
    err_sdpa = (sdpa16(q, k, v, H, D, offs, counts).float() - ref).abs().max().item()
    tol = 3 * ULP[dtype] * ref.abs().max().item()
    print(f"{what}: error {err:.3g} (gate {tol:.3g}), torch 16-bit SDPA {err_sdpa:.3g}")
    assert torch.isfinite(out).all()
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g}"
    assert err <= 1.5 * err_sdpa + 1e-6, f"{what}: error {err:.3g} vs torch 16-bit SDPA {err_sdpa:.3g}"
    for b, n in enumerate(counts):
        if n == 0:
            assert (out[b] == 0).all(), f"{what}: sample {b} has no keys: its rows must be exactly zero"


def _padded(kv, counts, L, fill=0.0):
    """the packed rows as a [B * L, .] buffer: sample b's keys first in its L rows, ``fill`` behind them"""
    pad = torch.full((len(counts) * L, kv.shape[1]), fill, device="cuda", dtype=kv.dtype)
    for b, (off, n) in enumerate(zip(_offsets(counts), counts)):
        pad[b * L:b * L + n] = kv[off:off + n]
    return pad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,D,counts", CASES, ids=IDS)
def test_cross_attention_accuracy_layouts_and_per_sample_equality(B, T, H, D, counts, dtype):
    from nunchaku_amd.ops import cross_attention

    hd, mk = H * D, max(counts)
    q, kv, k, v = _inputs(B, T, H, D, counts, dtype)
    offs = _offsets(counts)
    out = cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=mk)
    assert out.shape == (B, T, hd) and out.dtype == TD[dtype]
    _gate(out, q, k, v, H, D, offs, counts, dtype, f"({B},{T},{H},{D},{counts}) {dtype}")
    # two launches; a flat q with cu_seqlens; a looser bound on the counts
    assert torch.equal(cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=mk), out)
    assert torch.equal(cross_attention(q.flatten(0, 1), k, v, H, D, cu_seqlens=_cu(counts), max_keys=mk).view(B, T, hd), out)
    assert torch.equal(cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=320), out)
    if sum(counts) <= 320:
        assert torch.equal(cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts)), out)  # max_keys defaults to k.shape[0]
    # the padded form on the same keys: NaN behind every sample's keys
    L = mk + 5
    pad = _padded(kv, counts, L, NAN)
    po = torch.arange(0, B * L, L, dtype=torch.int32, device="cuda")
    pc = torch.tensor(counts, dtype=torch.int32, device="cuda")
    assert torch.equal(cross_attention(q, pad[:, :hd], pad[:, hd:], H, D, key_offsets=po, key_counts=pc, max_keys=mk), out)
    assert torch.equal(cross_attention(q, pad.view(B, L, -1)[..., :hd], pad.view(B, L, -1)[..., hd:], H, D, key_offsets=po, key_counts=pc, max_keys=mk), out)
    # every sample alone, its keys moved to row 0
    for b, (off, n) in enumerate(zip(offs, counts)):
        if n == 0:
            continue
        alone = kv[off:off + n].clone()
        one = cross_attention(q[b:b + 1], alone[:, :hd], alone[:, hd:], H, D, cu_seqlens=_cu([n]))
        assert torch.equal(one[0], out[b]), f"sample {b} of {counts}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,D,counts", [CASES[2], CASES[3], CASES[5]], ids=[IDS[2], IDS[3], IDS[5]])
def test_a_sample_sees_its_own_keys_only(B, T, H, D, counts, dtype):
    """rewriting another sample's keys and values with NaN, or rows inside no range, leaves a sample's output bit-equal"""
    from nunchaku_amd.ops import cross_attention

    hd, gap = H * D, 3
    q, kv, _, _ = _inputs(B, T, H, D, counts, dtype, seed=1)
    # ranges with `gap` rows in front of, between and behind them
    offs = [gap * (b + 1) + sum(counts[:b]) for b in range(B)]
    buf = torch.zeros(sum(counts) + gap * (B + 1), 2 * hd, device="cuda", dtype=TD[dtype])
    inside = torch.zeros(buf.shape[0], dtype=torch.bool, device="cuda")
    for b, (off, n, src) in enumerate(zip(offs, counts, _offsets(counts))):
        buf[off:off + n] = kv[src:src + n]
        inside[off:off + n] = True
    ko, kc = (torch.tensor(t, dtype=torch.int32, device="cuda") for t in (offs, counts))
    run = lambda t: cross_attention(q, t[:, :hd], t[:, hd:], H, D, key_offsets=ko, key_counts=kc, max_keys=max(counts))
    clean = run(buf)
    _gate(clean, q, buf[:, :hd], buf[:, hd:], H, D, offs, counts, dtype, f"ranges with gaps {counts} {dtype}")
    holes = buf.clone()
    holes[~inside] = NAN
    assert torch.equal(run(holes), clean), "rows inside no range were read"
    for b in range(B):
        other = buf.clone()
        for b2, (off, n) in enumerate(zip(offs, counts)):
            if b2 != b:
                other[off:off + n] = NAN
        got = run(other)
        assert torch.equal(got[b], clean[b]), f"sample {b} of {counts} changed with the other samples' keys"
        assert all(torch.isnan(got[b2]).all() for b2 in range(B) if b2 != b and counts[b2] > 0)  # (the poison was where those samples read)


MEMORY_CASES = [(1, 40, 1, 72, [70]), (2, 33, 1, 72, [1, 64]), CASES[0], CASES[1], CASES[2], CASES[3], CASES[6]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,H,D,counts", MEMORY_CASES, ids=[f"B{B}-T{T}-H{H}-D{D}-" + "_".join(map(str, c)) for B, T, H, D, c in MEMORY_CASES])
def test_nothing_outside_the_operands_is_read_or_written(B, T, H, D, counts, dtype):
    """Every poison value sits in memory this test owns: q's columns beyond H*D and its rows beyond B*T are NaN; the rows of the K/V buffer
    outside the ranges are NaN (K half) and 6e4 (V half), its columns beyond 2*H*D NaN; the output is a column slice of the first B*T rows of a
    larger sentinel-filled buffer.  D = 72 with H = 1: the missing half of the fifth K-step (channels 72..79) would be NaN columns of q and
    the first V columns (6e4 outside the ranges) of K, and an uncut store of the last O^T tile would land in out's sentinel columns."""
    from nunchaku_amd.ops import cross_attention

    hd, td, gap = H * D, TD[dtype], 3
    q, kv, k, v = _inputs(B, T, H, D, counts, dtype, seed=2)
    clean = cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=max(counts))
    big_q = torch.full((B * T + 40, _ceil128(hd) + 64), NAN, device="cuda", dtype=td)
    big_q[:B * T, :hd] = q.flatten(0, 1)[:, :hd]
    offs = [gap * (b + 1) + sum(counts[:b]) for b in range(B)]
    big_kv = torch.full((sum(counts) + gap * (B + 1) + 70, 2 * hd + 64), NAN, device="cuda", dtype=td)
    big_kv[:, hd:2 * hd] = 6e4
    for off, n, src in zip(offs, counts, _offsets(counts)):
        big_kv[off:off + n, :2 * hd] = kv[src:src + n]
    nrows = sum(counts) + gap * (B + 1)
    sentinel = -77.0
    big_o = torch.full((B * T + 33, hd + 128), sentinel, device="cuda", dtype=td)
    out = big_o[:B * T, 64:64 + hd].unflatten(0, (B, T))
    ko, kc = (torch.tensor(t, dtype=torch.int32, device="cuda") for t in (offs, counts))
    got = cross_attention(big_q[:B * T].unflatten(0, (B, T)), big_kv[:nrows, :hd], big_kv[:nrows, hd:2 * hd], H, D, key_offsets=ko, key_counts=kc,
                          max_keys=max(counts), out=out)
    assert got is out and torch.isfinite(out).all() and torch.equal(out, clean)
    assert (big_o[B * T:] == sentinel).all() and (big_o[:B * T, :64] == sentinel).all() and (big_o[:B * T, 64 + hd:] == sentinel).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,D", [(3, 112), (1, 72)])
def test_the_kernel_clamps_the_ranges_it_reads(H, D, dtype):
    """run on views of a larger buffer this test owns (finite rows behind the view), so that no version of the kernel can leave the allocation"""
    from nunchaku_amd.ops import cross_attention

    B, T, counts, hd = 2, 48, [50, 37], H * D
    q, _, _, _ = _inputs(B, T, H, D, counts, dtype, seed=3)
    g = torch.Generator(device="cuda").manual_seed(11)
    owner = torch.randn(sum(counts) + 400, 2 * hd, device="cuda", generator=g).to(TD[dtype])
    kv = owner[: sum(counts)]
    k, v = kv[:, :hd], kv[:, hd:]
    want = cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=320)
    _gate(want, q, k, v, H, D, _offsets(counts), counts, dtype, f"clamp baseline D={D} {dtype}")
    # a last entry beyond Nrows: the range is cut at Nrows
    cu = _cu(counts)
    cu[-1] += 17
    assert torch.equal(cross_attention(q, k, v, H, D, cu_seqlens=cu, max_keys=320), want)
    # an offset at or beyond Nrows, and a negative one: empty ranges
    ko = torch.tensor([0, sum(counts)], dtype=torch.int32, device="cuda")
    kc = torch.tensor(counts, dtype=torch.int32, device="cuda")
    got = cross_attention(q, k, v, H, D, key_offsets=ko, key_counts=kc, max_keys=320)
    assert torch.equal(got[0], want[0]) and (got[1] == 0).all()
    got = cross_attention(q, k, v, H, D, key_offsets=torch.tensor([0, -4], dtype=torch.int32, device="cuda"), key_counts=kc, max_keys=320)
    assert torch.equal(got[0], want[0]) and (got[1] == 0).all()
    # a decreasing pair: a negative count acts as 0
    cu = torch.tensor([0, 50, 20], dtype=torch.int32, device="cuda")
    got = cross_attention(q, k, v, H, D, cu_seqlens=cu, max_keys=320)
    assert torch.equal(got[0], want[0]) and (got[1] == 0).all()
    # a count above max_keys acts as max_keys
    ko = torch.tensor(_offsets(counts), dtype=torch.int32, device="cuda")
    cut = cross_attention(q, k, v, H, D, key_offsets=ko, key_counts=torch.tensor([30, 30], dtype=torch.int32, device="cuda"), max_keys=320)
    assert torch.equal(cross_attention(q, k, v, H, D, key_offsets=ko, key_counts=kc, max_keys=30), cut) and not torch.equal(cut, want)
    assert clamp_ranges(_offsets(counts), counts, sum(counts), 30) == [(0, 30), (50, 30)]
    # max_keys = 0: every sample is empty
    assert (cross_attention(q, k, v, H, D, key_offsets=ko, key_counts=kc, max_keys=0) == 0).all()


def _selection_probe(B, T, H, D, counts, dtype, amp=16.0, seed=0):
    """tests/test_gpu_dispatch_classes.py's every-key selection for per-sample ranges: k[n] is a vector of +-1 per head, row t of sample b asks for
    key (t + shift) mod count_b of its own range: q = amp * k[that key], so the row's own score is amp * sqrt(D) (>= 135) and every other
    one amp * (k_i . k_j) / sqrt(D), about +- amp.  Checked on the device in fp32: the own score leads all others of the sample by more than 40,
    i.e. every other probability is below e^-40 (fp16: rounds to 0; bf16: 320 of them are < 2^-24 of the winner's 1.0, so l = 1 and, with
    0.5 <= |v| < 2, O = v[winner] in fp32; what earlier chunks accumulated is rescaled by at most e^-40 and vanishes below the winner's ulp).
    out must then be the selected V row BIT FOR BIT.  With T >= count_b, shift 0 selects every key position of every chunk: first chunk, last
    chunk and the last valid position of a ragged chunk.  -> the smallest lead seen"""
    from nunchaku_amd.ops import cross_attention

    td, hd = TD[dtype], H * D
    N = sum(counts)
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + D)
    k = (torch.randint(0, 2, (N, hd), device="cuda", generator=g) * 2 - 1).to(td)
    v = ((torch.rand(N, hd, device="cuda", generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (N, hd), device="cuda", generator=g) * 2 - 1)).to(td)
    offs = _offsets(counts)
    margin = float("inf")
    for shift in range(0, max(counts), T):
        sel = torch.stack([(torch.arange(T, device="cuda") + shift) % n + off for off, n in zip(offs, counts)])  # [B, T] rows of k
        q = amp * k[sel]                                                                                        # [B, T, hd]
        for b, (off, n) in enumerate(zip(offs, counts)):
            s = torch.einsum("thd,nhd->htn", q[b].float().view(T, H, D), k[off:off + n].float().view(n, H, D)) * D ** -0.5
            idx = (sel[b] - off)[None, :, None].expand(H, T, 1)
            own = s.gather(2, idx).squeeze(2)
            lead = (own - s.scatter(2, idx, float("-inf")).max(dim=2).values).min().item() if n > 1 else float("inf")
            assert lead > 40, f"sample {b} shift {shift}: the selected key leads by {lead:.1f} only: the probe's precondition does not hold"
            margin = min(margin, lead)
        out = cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=max(counts))
        want = v[sel]
        assert torch.equal(out, want), f"shift {shift}: {int((out != want).any(dim=2).sum())} of {B * T} rows are not the selected key's V row"
    return margin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,D", [(2, 112), (3, 72), (1, 128)])
def test_every_key_position_of_every_chunk_is_selected(H, D, dtype):
    """300 keys: four full chunks and a ragged one of 44; 100 keys: a ragged second chunk; 320: five full chunks; 64: one"""
    margin = _selection_probe(4, 320, H, D, [300, 100, 320, 64], dtype)
    print(f"H={H} D={D} {dtype}: selection probe bit-exact, smallest lead {margin:.1f} (needs > 40)")
    margin = _selection_probe(2, 40, H, D, [300, 65], dtype, seed=1)  # T < count: shifts 0, 40, ..., 280
    print(f"H={H} D={D} {dtype}: selection probe with shifts bit-exact, smallest lead {margin:.1f} (needs > 40)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,D", [(2, 112), (2, 72)])
def test_softmax_edges(H, D, dtype):
    from nunchaku_amd.ops import cross_attention

    B, T, counts = 2, 64, [300, 100]
    N, offs = sum(counts), _offsets(counts)
    g = torch.Generator(device="cuda").manual_seed(7)
    td, hd = TD[dtype], H * D
    v = torch.randn(N, hd, device="cuda", generator=g).to(td)
    run = lambda q, k: cross_attention(q, k, v, H, D, cu_seqlens=_cu(counts), max_keys=300)
    # one key ahead of all others by more than 100 in score: q = 16 * ones, k_star = ones -> 16 * sqrt(D) >= 135, the others ~ 0.  The key sits
    # in the first chunk, in the last (ragged) chunk, and at the last valid position of the ragged chunk
    for star in ([17, 17], [260, 70], [299, 99]):
        k = (torch.randn(N, hd, device="cuda", generator=g) * 0.05).to(td)
        rows = [off + s for off, s in zip(offs, star)]
        k[rows] = 1.0
        q = torch.full((B, T, hd), 16.0, device="cuda", dtype=td)
        for b, (off, n) in enumerate(zip(offs, counts)):
            sc = torch.einsum("hd,nhd->hn", q[b, 0].float().view(H, D), k[off:off + n].float().view(n, H, D)) * D ** -0.5
            others = torch.cat([sc[:, :star[b]], sc[:, star[b] + 1:]], dim=1)
            assert (sc[:, star[b]] - others.max(dim=1).values).min().item() > 100
        out = run(q, k)
        _gate(out, q, k, v, H, D, offs, counts, dtype, f"one dominant key at {star} D={D} {dtype}")
        for b in range(B):
            assert torch.equal(out[b], v[rows[b]].expand(T, hd)), f"a row dominated by key {star[b]} returns that key's V row"
    # all keys of a sample equal: the mean of its V rows
    k_same = k[3].expand(N, hd).contiguous()
    q = torch.randn(B, T, hd, device="cuda", generator=g).to(td)
    out = run(q, k_same)
    for b, (off, n) in enumerate(zip(offs, counts)):
        mean = v[off:off + n].float().mean(dim=0)
        assert (out[b].float() - mean).abs().max().item() <= 3 * ULP[dtype] * mean.abs().max().item()
    _gate(out, q, k_same, v, H, D, offs, counts, dtype, f"all keys equal D={D} {dtype}")
    # scores near +-200 before the maximum is subtracted stay finite (fp16: exp(200) is far beyond the format)
    base = torch.randn(1, hd, device="cuda", generator=g)
    base = base / base.view(H, D).norm(dim=1).repeat_interleave(D)[None]  # unit norm per head
    amp = (200.0 * D ** 0.5) ** 0.5  # q . k = +-amp^2 -> scaled score +-200
    q = (base * amp).expand(T, hd).to(td).contiguous()
    q[T // 2:] *= -1
    q = q.expand(B, T, hd).contiguous()
    k = (base * amp).expand(N, hd).to(td).contiguous()
    k[1::2] *= -1  # (both signs in every chunk of every sample)
    k = (k.float() + torch.randn(N, hd, device="cuda", generator=g) * 0.05).to(td)
    sc = (q[0].float().view(T, H, D)[:, 0] @ k.float().view(N, H, D)[:, 0].T) * D ** -0.5
    assert sc.max() > 150 and sc.min() < -150
    out = run(q, k)
    _gate(out, q, k, v, H, D, offs, counts, dtype, f"scores near +-200 D={D} {dtype}")


def test_more_keys_and_other_head_dims_are_refused_and_the_call_can_be_captured():
    from nunchaku_amd.ops import cross_attention

    z = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    cu = _cu([321])
    with pytest.raises(NotImplementedError, match="at most 320"):
        cross_attention(z(1, 16, 256), z(321, 224), z(321, 224), 2, 112, cu_seqlens=cu)  # max_keys defaults to k.shape[0]
    with pytest.raises(NotImplementedError, match="head_dim=64"):
        cross_attention(z(1, 16, 256), z(4, 256), z(4, 256), 4, 64, cu_seqlens=_cu([4]))
    with pytest.raises(ValueError, match="cu_seqlens must live on q's device"):
        cross_attention(z(1, 16, 256), z(4, 224), z(4, 224), 2, 112, cu_seqlens=_cu([4]).cpu())
    # no host read of the ranges: the call is capturable, and a replay follows the counts the device holds at that time
    B, T, H, D, counts = 2, 48, 2, 72, [100, 37]
    q, kv, k, v = _inputs(B, T, H, D, counts, "bf16", seed=5)
    pad = _padded(kv, counts, 128)
    po = torch.arange(0, B * 128, 128, dtype=torch.int32, device="cuda")
    pc = torch.tensor(counts, dtype=torch.int32, device="cuda")
    out = torch.empty(B, T, H * D, device="cuda", dtype=torch.bfloat16)
    want = cross_attention(q, pad[:, :H * D], pad[:, H * D:], H, D, key_offsets=po, key_counts=pc, max_keys=128)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cross_attention(q, pad[:, :H * D], pad[:, H * D:], H, D, key_offsets=po, key_counts=pc, max_keys=128, out=out)
    graph.replay()
    assert torch.equal(out, want)
    pc.copy_(torch.tensor([64, 0], dtype=torch.int32, device="cuda"))
    graph.replay()
    assert torch.equal(out, cross_attention(q, pad[:, :H * D], pad[:, H * D:], H, D, key_offsets=po, key_counts=pc, max_keys=128)) and (out[1] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_key_buffer_without_rows_gives_zero_rows(dtype):
    """a packed condition with no text token in the whole batch: Nrows = 0, every range empty"""
    from nunchaku_amd.ops import cross_attention

    B, T, H, D = 2, 40, 3, 112
    q, _, _, _ = _inputs(B, T, H, D, [5, 5], dtype, seed=4)
    kv = torch.empty(0, 2 * H * D, device="cuda", dtype=TD[dtype])
    big_o = torch.full((B * T + 8, H * D + 128), -77.0, device="cuda", dtype=TD[dtype])
    out = big_o[:B * T, 64:64 + H * D].unflatten(0, (B, T))
    got = cross_attention(q, kv[:, :H * D], kv[:, H * D:], H, D, cu_seqlens=_cu([0, 0]), out=out)
    assert got is out and (out == 0).all()
    assert (big_o[B * T:] == -77.0).all() and (big_o[:B * T, :64] == -77.0).all() and (big_o[:B * T, 64 + H * D:] == -77.0).all()
    zo = torch.zeros(B, dtype=torch.int32, device="cuda")
    assert (cross_attention(q, kv[:, :H * D], kv[:, H * D:], H, D, key_offsets=zo, key_counts=zo + 7) == 0).all()


# ---- the module -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


def _layer(K, N, seed, bias, prefix):
    from oracle import svdq_oracle as O
    from tests.helpers import reference_state_dict

    L = O.make_svdq_layer(K, N, 32, seed=seed, dtype="bf16", bias=bias, cheap=True)
    return {prefix + k: v for k, v in reference_state_dict(L, "bf16").items()}


@pytest.mark.parametrize("heads,head_dim", [(2, 112), (4, 72)])
def test_module_equals_its_composition_from_the_public_pieces(heads, head_dim, strict_mode):
    from nunchaku_amd.models import SanaCrossAttention
    from nunchaku_amd.ops import cross_attention

    B, T, counts = 2, 70, [100, 37]
    m = SanaCrossAttention(heads, head_dim, device="cuda")
    dim, dp = m.dim, m.dim_pad
    assert (dim, dp) == ((224, 256) if head_dim == 112 else (288, 384))
    g = torch.Generator().manual_seed(dim)
    sd = {**_layer(dp, dp, 31, True, "q_linear."), **_layer(dp, dp, 32, True, "out_proj."),
          "kv_linear.weight": (torch.randn(2 * dim, dim, generator=g) * dim ** -0.5).to(torch.bfloat16), "kv_linear.bias": (torch.randn(2 * dim, generator=g) * 0.1).to(torch.bfloat16)}
    m.load_state_dict(sd, strict=True)
    x = torch.randn(B, T, dim, generator=g).to(torch.bfloat16).cuda()
    cond = torch.randn(sum(counts), dim, generator=g).to(torch.bfloat16).cuda()
    cu = _cu(counts)

    y = m(x, cond, None, cu)
    assert y.shape == (B, T, dim) and y.dtype == torch.bfloat16 and torch.isfinite(y).all() and y.float().abs().max() > 0.01
    assert torch.equal(m(x, cond, None, cu), y)                                                             # a second call
    assert torch.equal(m(x, cond, torch.arange(0, (B + 1) * T, T, dtype=torch.int32, device="cuda"), cu), y)  # cu_seqlens_img: its length only

    # the hand composition: q_linear -> kv_linear -> attention into a zero-tailed dim_pad buffer -> out_proj -> slice
    q = m.q_linear(F.pad(x, (0, dp - dim)))
    kv = m.kv_linear(cond)
    wide = torch.zeros(B, T, dp, device="cuda", dtype=torch.bfloat16)
    cross_attention(q, kv[:, :dim], kv[:, dim:], heads, head_dim, cu_seqlens=cu, max_keys=sum(counts), out=wide[..., :dim])
    assert torch.equal(y, m.out_proj(wide)[..., :dim])
    # the attention inside the module against the restatement, on the module's own projections
    _gate(wide[..., :dim], q, kv[:, :dim], kv[:, dim:], heads, head_dim, _offsets(counts), counts, "bf16", f"module ({heads},{head_dim})")

    # the padded form on the packed equivalent: NaN-free padding rows that the counts exclude
    L = 128
    cpad = _padded(cond, counts, L, 3.0).view(B, L, dim)
    kc = torch.tensor(counts, dtype=torch.int32, device="cuda")
    assert torch.equal(m.forward_padded(x, cpad, kc), y)
    # an empty sample: the attention gives zero rows, the layer out_proj's answer to them
    y0 = m.forward_padded(x, cpad, torch.tensor([counts[0], 0], dtype=torch.int32, device="cuda"))
    assert torch.equal(y0[0], y[0]) and torch.equal(y0[1], m.out_proj(torch.zeros(B, T, dp, device="cuda", dtype=torch.bfloat16))[1, :, :dim])
